// lm_reduce.hip -- the reductions behind the LM scalars and their hand-off to
// the host (fp64, gfx950).
//
// What the per-capture kernels leave per capture (parts, PartIdx) and per
// observation (obs_tg) is summed here: k_reduce_parts / k_lin_reduce, one
// 1024-thread block per LM scalar (element i -> thread i mod 1024, then one
// pairwise tree) and one thread per tag slot entry (a tag's observations in
// observation order); k_slot_norms, kNormBlocks blocks of 256 over the
// parameter slots, whose partials the last block to finish reduces over one
// tree; k_scale and k_lm_diag, one thread per slot.  With page-locked host
// words (hout) the results go straight to the host, and the last block to
// finish stores the sequence number the host polls; k_copy_out hands the
// parameters over the same way.
//
// k_cam_l_reduce and k_slot_norms_l (k_slot_norms' body, lm_slot_norms_body.h):
// the camera's l1, l2 slots of a problem that estimates them.
//
// Every sum that feeds an LM decision (cost, model cost change, step and
// gradient norms) is fixed-order: a fixed element -> thread assignment and a
// fixed tree, whichever block finishes last, and no atomics in any sum, so a
// solve is bit-identical run to run.
#include "lm_launch.h"
#include "lm_rows.h"

#include <algorithm>

namespace arslam {

namespace {

// Per tag slot: the gradient / column-norm sums over the tag's observations
// (obs_tg from k_linearize), in observation order.  Element e = 12 t + j.
__device__ __forceinline__ void tag_reduce_elem(const DevProblem &P, const double *__restrict__ obs_tg, long e,
                                                double *__restrict__ g, double *__restrict__ colnorm) {
  if (e >= 12L * P.nt) return;
  const int t = (int)(e / 12), j = (int)(e % 12);
  double s = 0.0;
  const int qa = P.tag_start[t], qb = P.tag_start[t + 1];
  // (obs_tg is tag-major: the tag's observations, in observation order, are
  // contiguous -- no index load in front of the sums' loads)
  for (int q0 = qa; q0 < qb; q0 += 32) {   // 32 loads in flight; summed in observation order
    double v[32];
#pragma unroll
    for (int u = 0; u < 32; ++u) v[u] = obs_tg[12L * min(q0 + u, qb - 1) + j];
#pragma unroll
    for (int u = 0; u < 32; ++u) s += (q0 + u < qb) ? v[u] : 0.0;
  }
  const long slot = slot_tag(P, t) + (j % 6);
  if (P.f_alias) {
    // (mixed e-set) a capture on the reduced side with a direct group: that
    // group's sums over its own pose (k_linearize) belong to this block; the
    // group's slot gets the total too, so its scale and LM diagonal are the block's
    const int d = P.f_alias[t];
    if (d >= 0) {
      double *dv = (j < 6 ? g : colnorm) + slot_cap(P, d) + (j % 6);
      s += *dv;
      *dv = P.slot_free[slot] ? s : 0.0;
    }
  }
  const double v = P.slot_free[slot] ? s : 0.0;
  if (j < 6) g[slot] = v; else colnorm[slot] = v;
}

// The hand-off of a launch's host words, by one thread of each block after the
// block's host stores were fenced at system scope: the block is counted on
// seq_done (a zeroed device int), and the last block to finish leaves the
// count zero again and stores the sequence number into *word, the page-locked
// word the host polls.  acq_rel at system scope: the last block acquires every
// other block's fenced host stores before its release of the word
__device__ __forceinline__ void last_block_stores_seq(int *seq_done, double *word, double seq) {
  if (__hip_atomic_fetch_add(seq_done, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_SYSTEM) == (int)gridDim.x - 1) {
    atomicExch(seq_done, 0);
    __hip_atomic_store(word, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// Deterministic single-block reduction of the per-capture partials.
// out[p] for p < NPART: sum (max for the *BAD flags); out[NPART] = F-side step^2,
// out[NPART+1] = F-side non-finite flag.
// One block per LM scalar p (deterministic: fixed element -> thread
// assignment, fixed tree); 8 loads in flight per thread.
__device__ __forceinline__ void reduce_parts_block(int p, const double *__restrict__ parts, int nc,
                                                   const double *__restrict__ fparts, int nfparts,
                                                   double *__restrict__ out, const int *__restrict__ flag,
                                                   double *red, double *__restrict__ hout,
                                                   int *seq_done = nullptr, double seq = 0.0,
                                                   double *__restrict__ save = nullptr) {
  const int t = threadIdx.x;
  const bool is_max = (p == P_YBAD || p == P_CBAD || p == NPART + 1);
  const double *src = p < NPART ? parts + (long)p * nc : fparts;
  const int len = p < NPART ? nc : (fparts ? nfparts : 0);
  const int stride = p < NPART ? 1 : 2, off0 = p < NPART ? 0 : p - NPART;
  double acc = 0.0;
  for (int i0 = t; i0 < len; i0 += 8 * 1024) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(long)stride * min(i0 + u * 1024, len - 1) + off0];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double w = (i0 + u * 1024 < len) ? v[u] : 0.0;
      acc = is_max ? fmax(acc, w) : acc + w;
    }
  }
  red[t] = acc;
  __syncthreads();
  for (int off = 512; off >= kWave; off >>= 1) {
    if (t < off) red[t] = is_max ? fmax(red[t], red[t + off]) : red[t] + red[t + off];
    __syncthreads();
  }
  if (t < kWave) {
    const double r = is_max ? wave_tree_max(red[t], kWave) : wave_tree_sum(red[t], kWave);
    if (t == 0) {
      out[p] = r;
      if (hout) hout[p] = r;
      if (save && p < 2) save[p] = r;   // (P_COST, P_FIXED)
    }
  }
  if (flag && p == 0 && t == 0) {   // rides along the step's one host read
    const int f = *flag;
    const double v[3] = {f > 0 ? 1.0 : 0.0,   // indefinite reduced system: an invalid LM step (max over ranks)
                         f < 0 ? 1.0 : 0.0,   // executor fault: an error, never a step (max over ranks)
                         (double)f};          // this rank's raw code, for the error message
    for (int q = 0; q < 3; ++q) {
      out[NPART + 2 + q] = v[q];
      if (hout) hout[NPART + 2 + q] = v[q];
    }
  }
  if (hout && t == 0) {
    // this block's host words out of its XCD's L2 (the blocks span XCDs);
    // then the last block to finish stores the sequence number
    __threadfence_system();
    if (seq_done && seq > 0.0) last_block_stores_seq(seq_done, hout + kHostSeq, seq);
  }
}

__global__ __launch_bounds__(1024) void k_reduce_parts(const double *__restrict__ parts, int nc,
                                                       const double *__restrict__ fparts,
                                                       int nfparts, double *__restrict__ out,
                                                       const int *__restrict__ flag,
                                                       double *__restrict__ hout, int *seq_done, double seq) {
  __shared__ double red[1024];
  reduce_parts_block(blockIdx.x, parts, nc, fparts, nfparts, out, flag, red, hout, seq_done, seq);
}

// The linearization's two reductions of k_linearize's output in one launch
// (they are independent): blocks 0 .. NPART+1 reduce the per-capture partials
// (k_reduce_parts), the rest sum the tag slots (tag_reduce_elem, 1024 slot entries each).
__global__ __launch_bounds__(1024) void k_lin_reduce(DevProblem P, const double *__restrict__ obs_tg,
                                                     double *__restrict__ g, double *__restrict__ colnorm,
                                                     const double *__restrict__ parts, double *__restrict__ out,
                                                     double *__restrict__ hout, double *__restrict__ save) {
  __shared__ double red[1024];
  if ((int)blockIdx.x < NPART + 2)
    reduce_parts_block(blockIdx.x, parts, P.nc, nullptr, 0, out, nullptr, red, hout, nullptr, 0.0, save);
  else
    tag_reduce_elem(P, obs_tg, (long)(blockIdx.x - (NPART + 2)) * 1024 + threadIdx.x, g, colnorm);
}

// (diag: also the LM diagonal clamp(s^2 colnorm, dmin, dmax) from the new scale: k_lm_diag's work)
__global__ void k_scale(long n, const unsigned char *__restrict__ free_, const double *__restrict__ colnorm,
                        int jacobi, double *__restrict__ scale, double dmin, double dmax, double *__restrict__ diag) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // jacobian_scaling = 1 / (1 + sqrt(SquaredColumnNorm)) at iteration 0
  const double sv = free_[i] ? (jacobi ? 1.0 / (1.0 + sqrt(colnorm[i])) : 1.0) : 0.0;
  scale[i] = sv;
  if (diag) diag[i] = fmin(fmax(sv * sv * colnorm[i], dmin), dmax);
}

__global__ void k_lm_diag(long n, const double *__restrict__ scale, const double *__restrict__ colnorm,
                          double dmin, double dmax, double *__restrict__ diag) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double d = scale[i] * scale[i] * colnorm[i];   // squared column norm of J * diag(s)
  diag[i] = fmin(fmax(d, dmin), dmax);
}

// Norms over free parameter slots, split into capture slots (out[0..2]) and
// camera + tag slots (out[3..5]): max |g|, sum g^2, sum x^2.  The split lets
// the capture-sharded path reduce only the disjoint capture part across ranks.

// (the body: lm_slot_norms_body.h)
__global__ __launch_bounds__(256) void k_slot_norms(long n, long cap_lo, long cap_hi,
                                                    const unsigned char *__restrict__ free_,
                                                    const unsigned char *__restrict__ f_own,
                                                    double *__restrict__ g, double *__restrict__ colnorm,
                                                    const double *__restrict__ red,
                                                    const double *__restrict__ x,
                                                    double *__restrict__ out,
                                                    double *__restrict__ hout, const double *__restrict__ scale,
                                                    double dmin, double dmax, double *__restrict__ diag, double seq) {
  constexpr bool kL = false;
  constexpr const double *lred = nullptr;
#include "lm_slot_norms_body.h"
}

// ... of a problem whose l1, l2 are estimated
__global__ __launch_bounds__(256) void k_slot_norms_l(long n, long cap_lo, long cap_hi,
                                                      const unsigned char *__restrict__ free_,
                                                      const unsigned char *__restrict__ f_own,
                                                      double *__restrict__ g, double *__restrict__ colnorm,
                                                      const double *__restrict__ red,
                                                      const double *__restrict__ x,
                                                      double *__restrict__ out,
                                                      double *__restrict__ hout, const double *__restrict__ scale,
                                                      double dmin, double dmax, double *__restrict__ diag, double seq,
                                                      const double *__restrict__ lred) {
  constexpr bool kL = true;
#include "lm_slot_norms_body.h"
}

// The camera's l sums: block i (of 4) adds k_linearize_est's partials
// lparts[i nc .. (i + 1) nc) -- J_l1'r, J_l2'r, |J_l1|^2, |J_l2|^2 per capture --
// capture c in thread c mod 256, then one pairwise tree: a fixed order.
__global__ __launch_bounds__(256) void k_cam_l_reduce(const double *__restrict__ lparts, int nc,
                                                      double *__restrict__ lred) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const double *src = lparts + (long)blockIdx.x * nc;
  double acc = 0.0;
  for (int i = t; i < nc; i += 256) acc += src[i];
  red[t] = acc;
  __syncthreads();
  for (int off = 128; off >= kWave; off >>= 1) {
    if (t < off) red[t] += red[t + off];
    __syncthreads();
  }
  if (t < kWave) {
    const double r = wave_tree_sum(red[t], kWave);
    if (t == 0) lred[blockIdx.x] = r;
  }
}

}  // namespace

// The parameter download on one rank: a kernel stores x straight into the
// page-locked host buffer and the last block to finish stores the sequence
// number after every block's stores were made visible at system scope (the
// host polls that word, as in the LM loop) -- no copy engine, no event.
__global__ __launch_bounds__(256) void k_copy_out(const double *__restrict__ src, long n, double *__restrict__ dst,
                                                  int *seq_done, double *word, double seq) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = src[i];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) last_block_stores_seq(seq_done, word, seq);
}

void launch_lin_reduce(const DevProblem &P, const double *obs_tg, double *g, double *colnorm,
                       const double *parts, double *out, hipStream_t s, double *hout, double *save) {
  const unsigned tag_blocks = (unsigned)((12L * P.nt + 1023) / 1024);
  hipLaunchKernelGGL(k_lin_reduce, dim3(NPART + 2 + tag_blocks), dim3(1024), 0, s, P, obs_tg, g, colnorm, parts,
                     out, hout, save);
}

void launch_scale(const DevProblem &P, const double *colnorm, int jacobi, double *scale, hipStream_t s,
                  const LmDiagArgs *ld) {
  hipLaunchKernelGGL(k_scale, dim3((unsigned)((P.n + 255) / 256)), dim3(256), 0, s, P.n, P.slot_free,
                     colnorm, jacobi, scale, ld ? ld->dmin : 0.0, ld ? ld->dmax : 0.0, ld ? ld->diag : nullptr);
}

void launch_lm_diag(const DevProblem &P, const double *scale, const double *colnorm, double dmin,
                    double dmax, double *diag, hipStream_t s) {
  hipLaunchKernelGGL(k_lm_diag, dim3((unsigned)((P.n + 255) / 256)), dim3(256), 0, s, P.n, scale,
                     colnorm, dmin, dmax, diag);
}

void launch_reduce_parts(const double *parts, int nc, const double *fparts, int nfparts, double *out,
                         hipStream_t s, const int *flag, double *hout, int *seq_done, double seq) {
  hipLaunchKernelGGL(k_reduce_parts, dim3(NPART + 2), dim3(1024), 0, s, parts, nc, fparts, nfparts, out, flag, hout,
                     seq_done, seq);
}

void launch_slot_norms(const DevProblem &P, const double *red, double *g, double *colnorm, const double *x,
                       double *out, hipStream_t s, double *hout, const LmDiagArgs *ld, double seq,
                       const DevCamL *cl) {
  // out[0..5] results, out[7] the block count (zero between launches), out[8..] the per-block partials
  if (cl) {   // l1, l2 estimated: their sums first, then the instance that reads them
    hipLaunchKernelGGL(k_cam_l_reduce, dim3(4), dim3(256), 0, s, cl->lparts, P.nc, cl->lred);
    hipLaunchKernelGGL(k_slot_norms_l, dim3(kNormBlocks), dim3(256), 0, s, P.n, 3L, 3L + 6L * P.nc, P.slot_free,
                       P.f_own, g, colnorm, red, x, out, hout, ld ? ld->scale : nullptr, ld ? ld->dmin : 0.0,
                       ld ? ld->dmax : 0.0, ld ? ld->diag : nullptr, seq, cl->lred);
    return;
  }
  hipLaunchKernelGGL(k_slot_norms, dim3(kNormBlocks), dim3(256), 0, s, P.n, 3L, 3L + 6L * P.nc, P.slot_free, P.f_own, g,
                     colnorm, red, x, out, hout, ld ? ld->scale : nullptr, ld ? ld->dmin : 0.0,
                     ld ? ld->dmax : 0.0, ld ? ld->diag : nullptr, seq);
}

void launch_copy_out(const double *src, long n, double *dst, int *seq_done, double *word, double seq, hipStream_t s) {
  const unsigned blocks = (unsigned)std::min<long>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(k_copy_out, dim3(std::max(blocks, 1u)), dim3(256), 0, s, src, n, dst, seq_done, word, seq);
}

}  // namespace arslam
