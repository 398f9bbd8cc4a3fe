// lm_launch.h -- the launch wrappers of the LM step's kernels, by the file
// that holds them (lm_linearize.hip, lm_schur.hip, lm_step.hip, lm_reduce.hip,
// lm_exchange.hip), and the small argument structs they take.  Called by the
// LM driver (lm_solve.hip, lm_load.hip, lm_covariance.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdexcept>

#include "llt_plan.h"     // ExecReset (launch_schur carries the executors' reset), LmDiagArgs
#include "lm_problem.h"

namespace arslam {

// ---- lm_linearize.hip ----
// (cl: a problem whose l1, l2 are estimated -- the instances that also store
// the rows' l columns, cl->jrows_l, and the per-capture partials of the l
// gradient and column norms, cl->lparts; null: the launches it has always been)
void launch_linearize(const DevProblem &P, const double *x, double *g, double *colnorm,
                      double *obs_tg, double *parts, hipStream_t s, const DevCamL *cl = nullptr);

// ---- lm_schur.hip ----
// k_schur<true>'s dynamic-LDS attribute on the current device (once per device)
void set_schur_big_lds_attribute();
// (prep = true: k_prep_reduced's diagonal work is done by the gather itself --
// single rank only, where the gathered S is final)
// (zero_tiles: the first zero_tiles 64x64 tiles of S are cleared by extra
// k_schur blocks before the gather writes S)
// (er: the persistent executors' reset rides along in k_schur's blocks past
// the tiles; only with P.nc > 0)
void launch_schur(const DevProblem &P, const double *x, const double *scale, const double *diag,
                  double radius, double *S, hipStream_t s, bool prep = false, long zero_tiles = 0,
                  const ExecReset *er = nullptr);
// launch_schur's second half alone (one rank, prep mode): the gather of the
// local systems already in P.slab into a cleared S, with the diagonal's D^2
// and the padding / rhs rows (the covariance fills the slab itself)
void launch_schur_gather(const DevProblem &P, const double *diag, double radius, double *S, hipStream_t s);
// (which: -1 every row; 0 / 1 only the rows of tile columns of that class)
void launch_prep_reduced(const DevProblem &P, const double *diag, double radius, double *S,
                         hipStream_t s, int which = -1);
// test hook: S[row, row] = v (arslam_lm_debug_force_indefinite)
void debug_set_reduced_diag(const DevProblem &P, double *S, long row, double v, hipStream_t s);
// k_schur's phase clocks, 16 words (zeros unless built with -DARSLAM_SCHUR_STAMPS)
void debug_read_schur_stamps(unsigned long long *out);

// ---- lm_schur_cam.hip ----
// A problem whose l1, l2 are estimated (one rank, prep mode), after launch_schur on the same stream: the e-blocks' borders of the
// Schur complement for the two l columns (k_schur_cam, from jrows, cl.jrows_l and
// the cap_ui k_schur left) and their sums into reduced rows cam_row + 1,
// cam_row + 2 and the rhs row, with the rows' D_f^2.
void launch_schur_cam(const DevProblem &P, const DevCamL &cl, const double *scale, const double *diag, double radius, double *S,
                      hipStream_t s);
// The second half of launch_schur_cam on its own: the sums of the borders in
// cl.cam_slab into S (k_schur_cam_gather), whoever stored them there -- the
// covariance's elimination assembles its border with it (cov_lens.hip).
void launch_schur_cam_gather(const DevProblem &P, const DevCamL &cl, const double *diag, double radius, double *S,
                             hipStream_t s);
// debug: reduced rows cam_row .. cam_row + 2 of S against every reduced column
// and the rhs, out[b (nR + 1) + col] (device memory)
void debug_cam_rows(const DevProblem &P, double *S, double *out, hipStream_t s);
// debug: the padded reduced system, N x N with both triangles, 0 where the factor
// has no tile (device memory)
void debug_reduced_dense(const DevProblem &P, const double *S, double *out, hipStream_t s);

// ---- lm_step.hip ----
void launch_backsub(const DevProblem &P, const double *x, const double *scale, const double *diag,
                    double radius, const double *yF, double *xc, double *parts, hipStream_t s,
                    bool reuse_ui = false, bool with_cost = false, const DevCamL *cl = nullptr);
// candidate f-side slots: xc = x - s yF on reduced rows, xc = x elsewhere (every
// f-side slot is written); fparts: 2 per 256 reduced rows
void launch_update_f(const DevProblem &P, const double *x, const double *scale, const double *yF,
                     double *xc, double *fparts, hipStream_t s);
void launch_cost(const DevProblem &P, const double *x, double *parts, hipStream_t s);

// ---- lm_reduce.hip ----
// (hout, in launch_lin_reduce, launch_reduce_parts and launch_slot_norms:
// page-locked host words that also receive the results, so a single-rank solve
// needs no device-to-host copy for them; each writer releases them at system
// scope)
// hout[kHostSeq]: the launch's sequence number, stored last (a host-memory flag:
// a ~8 us kernel-to-host round trip against ~13 us for an event query on
// MI355X, tools/sync_bench.hip)
constexpr int kHostSeq = 15;
// k_slot_norms' blocks (each one's six partials are reduced by the last to finish)
#ifndef ARSLAM_NORM_BLOCKS
#define ARSLAM_NORM_BLOCKS 64
#endif
constexpr int kNormBlocks = ARSLAM_NORM_BLOCKS;
static_assert(kNormBlocks <= 256 && (kNormBlocks & (kNormBlocks - 1)) == 0, "k_slot_norms: one 256-thread tree");

// k_linearize's reductions in one launch: the per-capture partials into
// out[0..NPART+1] (launch_reduce_parts without fparts) and the tag slots' g and colnorm
// (save: also the cost and fixed cost, out[P_COST], out[P_FIXED], into save[0..1])
void launch_lin_reduce(const DevProblem &P, const double *obs_tg, double *g, double *colnorm,
                       const double *parts, double *out, hipStream_t s, double *hout = nullptr,
                       double *save = nullptr);
// reduce per-capture partials [NPART][nc] (+ f-slot partials) into out[NPART]
// (flag: also out[NPART + 2] = indefinite (flag > 0), out[NPART + 3] = executor
// fault (flag < 0), out[NPART + 4] = the raw flag)
// (seq_done, seq > 0: with hout, the last block to finish also stores seq into
// hout[kHostSeq] after every block's host words -- the LM loop's host polls that
// word instead of an event; seq_done: a zeroed device int, left zero again)
void launch_reduce_parts(const double *parts, int nc, const double *fparts, int nfparts,
                         double *out, hipStream_t s, const int *flag = nullptr,
                         double *hout = nullptr, int *seq_done = nullptr, double seq = 0.0);
// (ld: also the LM diagonal from the new scale, ld->diag / dmin / dmax)
void launch_scale(const DevProblem &P, const double *colnorm, int jacobi, double *scale,
                  hipStream_t s, const LmDiagArgs *ld = nullptr);
void launch_lm_diag(const DevProblem &P, const double *scale, const double *colnorm, double dmin,
                    double dmax, double *diag, hipStream_t s);
// The camera slots of g and colnorm from the reduced partials red (P_GF, P_CF),
// then the norms over free parameter slots: out[0..2] = max|g|, sum g^2, sum x^2
// over capture slots, out[3..5] the same over camera + tag slots.  out[7] is
// the launch's block count (must be zero before the first launch), out[8..]
// its per-block partials.
// (ld: also the LM diagonal clamp(s^2 colnorm) of every slot from ld->scale, into ld->diag)
// (seq > 0: with hout, the last block stores seq into hout[kHostSeq] after the results)
// (cl: a problem whose l1, l2 are estimated -- launch_linearize's l partials
// are summed into cl->lred[0..3] first, and camera slots 1, 2 of g and
// colnorm, the norms and the LM diagonal take them from there)
void launch_slot_norms(const DevProblem &P, const double *red, double *g, double *colnorm, const double *x,
                       double *out, hipStream_t s, double *hout = nullptr, const LmDiagArgs *ld = nullptr,
                       double seq = 0.0, const DevCamL *cl = nullptr);
// x[0..n) into the page-locked dst; the last block stores seq into *word (page-locked,
// after the data; seq_done: a zeroed device int, left zero again)
void launch_copy_out(const double *src, long n, double *dst, int *seq_done, double *word, double seq, hipStream_t s);

// ---- lm_exchange.hip ----
// multi-rank: the backward solve's y before its all-reduce: this rank's
// subtree rows kept, the top rows kept on rank 0 only, every other row 0
// (keep_top: the top rows kept on every rank -- every rank holds the top's y)
void launch_mask_y(const DevProblem &P, double *yF, int rank, hipStream_t s, bool keep_top = false);
// dst[i] = f_own[first + i] ? src[i] : 0 for i < count (several ranks: the values this rank holds)
void launch_own_copy(const DevProblem &P, long first, long count, const double *src, double *dst, hipStream_t s);
// multi-rank exchange buffers: up to 4 segments packed at offsets off[] of one buffer
struct PackSegs {
  int n = 0;
  double *p[4] = {nullptr, nullptr, nullptr, nullptr};
  long len[4] = {0, 0, 0, 0}, off[4] = {0, 0, 0, 0};
  void add(double *ptr, long count) {
    p[n] = ptr;
    len[n] = count;
    off[n] = n ? off[n - 1] + len[n - 1] : 0;
    ++n;
  }
  long total() const { return n ? off[n - 1] + len[n - 1] : 0; }
};
void launch_pack(const PackSegs &sg, double *buf, bool unpack, hipStream_t s);
// tail[0..m) = g[idx], tail[m..2m) = cn[idx], tail[2m..2m+2) = red[P_GF], red[P_CF] (unpack: the reverse):
// the top tags' linearization sums riding in front of the top tiles' all-reduce
void launch_top_tail(const int *idx, int m, double *g, double *cn, double *red, double *tail, bool unpack,
                     hipStream_t s);
// all-gather of up to kAgFields scalars src[idx[f]] through one SUM all-reduce of
// ag[nranks][kAgFields] (launch_ag_put), combined in rank order by sum, or max
// where bit f of `max` is set (launch_ag_reduce, into dst[idx[f]])
constexpr int kAgFields = 32;
struct AgFields {
  int n = 0;
  int idx[kAgFields] = {};
  unsigned max = 0;
  void add(int i, bool is_max) {
    if (n >= kAgFields) throw std::logic_error("AgFields: more than kAgFields scalars");
    if (is_max) max |= 1u << n;
    idx[n++] = i;
  }
};
void launch_ag_put(const double *src, const AgFields &fl, double *ag, int nranks, int rank, hipStream_t s);
// (several ranks) device ranges stored into page-locked host words by the
// all-gather's combining launch itself, then the sequence number the host
// polls (as one rank's reductions do): no copy launches, no event
struct HostOut {
  const double *src[3] = {};
  double *dst[3] = {};
  int len[3] = {};
  int n = 0;
  double *seq_word = nullptr;
  double seq = 0.0;
  void add(const double *s, double *d, int l) {
    if (n >= 3) throw std::logic_error("HostOut: more than 3 ranges");
    src[n] = s;
    dst[n] = d;
    len[n++] = l;
  }
};
void launch_ag_reduce(const double *ag, const AgFields &fl, double *dst, int nranks, hipStream_t s,
                      const HostOut *ho = nullptr);

}  // namespace arslam
