// lm_handle.h -- the handle behind the C-ABI of include/arslam_lm.h: its
// own buffers and timers (HIP_CHECK and DevBuf are hip_host.h's), and
// `struct arslam_lm` with every member.  The methods'
// bodies live in lm_load.hip (load, upload, append, value reload), lm_solve.hip
// (the trust-region loop, its stages, the linearization), lm_covariance.hip,
// lm_evaluate.hip (arslam_lm_evaluate*, with its own entry points),
// lm_cov_capi.hip (the covariance entry points) and lm_capi.hip (the other
// extern "C" entry points); only those include this header.
#pragma once
#include "hip_host.h"
#include "host_threads.h"
#include "llt_plan.h"
#include "lm_cov.h"
#include "lm_evaluate.h"
#include "lm_launch.h"
#include "lm_problem.h"
#include "loss.h"
#include "arslam_lm.h"
#include "arslam_lm_debug.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <thread>
#include <unordered_set>
#include <vector>

namespace arslam {
namespace lmh {   // the LM handle's host helpers

using Error = arslam::ApiError;
using arslam::DevBuf;

#define NCCL_CHECK(expr)                                                                     \
  do {                                                                                       \
    ncclResult_t _r = (expr);                                                                \
    if (_r != ncclSuccess)                                                                   \
      throw Error(ARSLAM_E_COMM, std::string(#expr) + ": " + ncclGetErrorString(_r));       \
  } while (0)

inline void fail_if(bool cond, int code, const std::string &msg) {
  if (cond) throw Error(code, msg);
}

inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The debug switches of the load and solve paths, read once per process (at
// the first handle's creation), never inside a loop.
struct DebugEnv {
  const char *dag_trace = std::getenv("ARSLAM_DAG_TRACE");   // dump one k_factor_dag task timeline to this path
  int dag_trace_skip = std::getenv("ARSLAM_DAG_TRACE_SKIP") ? std::atoi(std::getenv("ARSLAM_DAG_TRACE_SKIP")) : 0;
  bool setup_profile = std::getenv("ARSLAM_SETUP_PROFILE") != nullptr;    // setup phases to stderr
  bool write_back_dma = std::getenv("ARSLAM_WRITE_BACK_DMA") != nullptr;   // A/B: the copy engine
};
inline const DebugEnv &debug_env() {
  static const DebugEnv e;
  return e;
}

// decode the persistent executors' negative flags (lm_solve.hip); for a
// timed-out wait of k_factor_dag also what its fault record says
std::string executor_fault_message(int code, int rank, int iteration, const arslam::LltPlan &plan, hipStream_t s);

// page-locked host words: a D2H copy into them stays asynchronous
struct PinnedBuf {
  double *p = nullptr;
  size_t cap = 0;
  void alloc(size_t count) {   // grows only (by half again: page-locking is slow); kept across solves
    if (count <= cap) return;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = count + count / 2;
    HIP_CHECK(hipHostMalloc(&p, want * sizeof(double), hipHostMallocDefault));
    cap = want;
  }
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
};

// The problem's uploaded arrays: one grow-only device allocation, one
// page-locked host image, one host->device copy per load (instead of a
// pageable copy and a driver staging pass per array).
struct UploadArena {
  char *dev = nullptr, *host = nullptr;
  size_t dev_cap = 0, host_cap = 0;
  struct Piece { void **dst; const void *src; size_t bytes, off; };
  std::vector<Piece> pieces;
  hipEvent_t copied = nullptr;   // the last commit's transfer has read the host image
  template <class T>
  void add(T **dst, const T *src, size_t count) { pieces.push_back({reinterpret_cast<void **>(dst), src, count * sizeof(T), 0}); }
  // lay the pieces out, copy them into the host image and enqueue the one
  // transfer; the sources may go out of scope once this returns, the image
  // stays untouched until the caller's next stream sync
  void commit(hipStream_t s) {
    // the previous transfer may still be reading the image (a load with no
    // reduced system has no stream sync before the next upload)
    if (copied) HIP_CHECK(hipEventSynchronize(copied));
    size_t used = 0;
    for (Piece &p : pieces) {
      p.off = used;
      used += (std::max<size_t>(p.bytes, 1) + 255) & ~size_t(255);
    }
    if (used > host_cap) {
      if (host) (void)hipHostFree(host);
      host = nullptr;
      host_cap = 0;
      HIP_CHECK(hipHostMalloc(&host, used + used / 2, hipHostMallocDefault));
      host_cap = used + used / 2;
    }
    if (used > dev_cap) {
      if (dev) (void)hipFree(dev);
      dev = nullptr;
      dev_cap = 0;
      HIP_CHECK(hipMalloc(&dev, used + used / 2));
      dev_cap = used + used / 2;
    }
    for (Piece &p : pieces) {
      if (p.bytes) std::memcpy(host + p.off, p.src, p.bytes);
      *p.dst = dev + p.off;
    }
    if (used) {
      HIP_CHECK(hipMemcpyAsync(dev, host, used, hipMemcpyHostToDevice, s));
      if (!copied) HIP_CHECK(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
      HIP_CHECK(hipEventRecord(copied, s));
    }
    pieces.clear();
  }
  ~UploadArena() {
    if (copied) (void)hipEventDestroy(copied);
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
  }
};

struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
  double acc_ms = 0.0;
  bool pending = false;
  bool on = true;   // options.phase_timing
  void init() {
    if (!a) {
      // timing only (read after the stream's sync): no system-scope fence at
      // the record -- its cache writeback and invalidation sat between the
      // kernels it brackets (~6 us each side of the factorization)
      HIP_CHECK(hipEventCreateWithFlags(&a, hipEventDisableSystemFence));
      HIP_CHECK(hipEventCreateWithFlags(&b, hipEventDisableSystemFence));
    }
  }
  void start(hipStream_t s) {
    if (on) HIP_CHECK(hipEventRecord(a, s));
  }
  void stop(hipStream_t s) {
    if (!on) return;
    HIP_CHECK(hipEventRecord(b, s));
    pending = true;
  }
  void collect() {  // call after the stream was synchronized (or its flag seen: b may still be pending)
    if (!pending) return;
    float ms = 0.f;
    HIP_CHECK(hipEventSynchronize(b));
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    acc_ms += ms;
    pending = false;
  }
  void destroy() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    a = b = nullptr;
  }
};

enum { PH_LIN, PH_SCHUR, PH_CHOL, PH_SOLVE, PH_BACK, PH_COST, PH_FAC0, PH_FAC1, PH_N };

}  // namespace lmh
}  // namespace arslam
using namespace arslam::lmh;   // (this header is private to the lm_*.hip files)

struct arslam_lm {
  arslam_lm_options opt;

  // ---- pointer-keyed problem (Ceres API mirror) ----
  double *camera_ptr = nullptr;
  std::unordered_map<double *, int> cap_of, tag_of;
  std::vector<double *> cap_ptrs, tag_ptrs;
  std::vector<int> pk_obs_cap, pk_obs_tag;
  std::vector<double> pk_corners;
  // each residual block's loss (arslam_lm_add_residual_block_loss; the default
  // loss for arslam_lm_add_residual_block).  Blocks are only ever appended, or
  // all dropped by arslam_lm_reset (a full load follows), so a resident
  // problem's losses never go stale under the values-only path, and the
  // append path uploads the grown arrays with the grown problem.
  std::vector<unsigned char> pk_loss_kind;
  std::vector<double> pk_loss_a;
  int def_loss_kind = ARSLAM_LOSS_NONE;   // arslam_lm_set_loss
  double def_loss_a = 0.0;
  std::vector<unsigned char> soa_loss_kind;   // arslam_lm_load_soa's default loss, per observation
  std::vector<double> soa_loss_a;
  // the default loss for each of n_obs observations (null arrays: NONE)
  arslam::ObsLoss default_obs_loss(int n_obs) {
    if (def_loss_kind == ARSLAM_LOSS_NONE || n_obs <= 0) return arslam::ObsLoss{};
    soa_loss_kind.assign(n_obs, (unsigned char)def_loss_kind);
    soa_loss_a.assign(n_obs, def_loss_a);
    return arslam::ObsLoss{soa_loss_kind.data(), soa_loss_a.data()};
  }
  // each residual block's tag side (arslam_lm_add_residual_block_sized; the
  // handle's default side for the other two), beside pk_loss_* and under the
  // same rules: bound when the block is added, never changed afterwards
  std::vector<double> pk_size;
  double def_tag_size = ARSLAM_DEFAULT_TAG_SIZE;   // arslam_lm_set_tag_size
  // the camera model of the next load (arslam_lm_set_camera_model): the loaded
  // problem's is DevProblem::camera_radial, and a change drops that problem
  int camera_model = ARSLAM_CAMERA_PINHOLE;
  // "estimate the distortion" (arslam_lm_set_estimate_distortion): a property
  // of the handle like the camera model, bound at the next load; it takes
  // effect under ARSLAM_CAMERA_RADIAL only (est_active), and the loaded
  // problem's is est_loaded (a free camera besides): CL beside P
  int estimate_distortion = 0;
  bool est_active() const { return estimate_distortion != 0 && camera_model == ARSLAM_CAMERA_RADIAL; }
  // what the switch does not cover, refused before the handle changes
  void est_check_load(const arslam_soa_problem *p_in) const;
  bool est_loaded = false;
  arslam::DevCamL CL{};
  const arslam::DevCamL *cl() const { return est_loaded ? &CL : nullptr; }
  std::vector<int> camg_start;    // DevCamL::camg_start, camg_items (x, y interleaved)
  std::vector<int> camg_items;
  int *u_camg_start = nullptr;
  int2 *u_camg_items = nullptr;
  DevBuf<double> d_jrows_l, d_cam_slab, d_lparts, d_lred;
  std::vector<double> soa_size;   // arslam_lm_load_soa*'s tag sides, per observation
  // the side of each observation's tag from the per-tag sides (null: the
  // handle's default for every tag); null when every side is the default
  const double *obs_sizes(const arslam_soa_problem *p, const double *tag_size) {
    if (!tag_size && def_tag_size == ARSLAM_DEFAULT_TAG_SIZE) return nullptr;
    soa_size.resize(p->n_obs > 0 ? p->n_obs : 0);
    for (int b = 0; b < p->n_obs; ++b) soa_size[b] = tag_size ? tag_size[p->obs_tag[b]] : def_tag_size;
    return soa_size.data();
  }
  std::unordered_set<double *> constant;
  // the caller's {kind, index} of a pointer-keyed block (the camera: index 0); throws for a pointer that is no block
  void pk_block(const double *block, int *kind, int *index) const {
    double *key = const_cast<double *>(block);
    const auto ci = cap_of.find(key);
    const auto ti = tag_of.find(key);
    fail_if(key != camera_ptr && ci == cap_of.end() && ti == tag_of.end(), ARSLAM_E_INVALID_ARG,
            "parameter block is not part of the problem");
    *kind = key == camera_ptr ? ARSLAM_BLOCK_CAMERA : ci != cap_of.end() ? ARSLAM_BLOCK_CAPTURE : ARSLAM_BLOCK_TAG;
    *index = *kind == ARSLAM_BLOCK_CAMERA ? 0 : *kind == ARSLAM_BLOCK_CAPTURE ? ci->second : ti->second;
  }
  // The pointer-keyed structure (blocks, residuals, constants) changed since
  // the last load: arslam_lm_solve reloads; otherwise it reuses the resident
  // problem, plan and buffers and uploads only the parameter values.
  bool pk_dirty = true;

  // ---- loaded problem ----
  bool loaded = false;
  arslam_soa_problem soa{};
  int nc = 0, nt = 0, nb = 0;
  long n = 0, nR = 0, N = 0;
  bool has_f = false;
  std::vector<unsigned char> slot_free;
  std::vector<double> x0;   // initial slots
  long nb_global = 0;       // observations over all ranks
  double setup_s = 0.0;     // host structure + ordering + plan + upload of the last load (or value reload)
  double setup_phase[5] = {0, 0, 0, 0, 0};   // the last full load's phases (summary.setup_phase_s)
  double comm_bytes = 0.0;  // bytes this rank all-reduced (RCCL or the host callback) since the count was reset
  long comm_calls = 0;      // ... and the collectives that carried them
  arslam::DevProblem P{};
  hipStream_t stream = nullptr;
  int device = 0;

  // uploaded arrays (pointers into `upload`, re-laid out by every load)
  UploadArena upload;
  int *u_cap_start = nullptr, *u_obs_tag = nullptr, *u_obs_lblk = nullptr, *u_cap_blk_start = nullptr,
      *u_blk_tag = nullptr, *u_tag_start = nullptr, *u_obs_tpos = nullptr, *u_tag_row = nullptr,
      *u_row_slot = nullptr, *u_fslot_row = nullptr, *u_dest_start = nullptr, *u_big_caps = nullptr;
  unsigned char *u_f_own = nullptr;
  unsigned char *u_cap_kind = nullptr;   // ARSLAM_ELIM_MIXED: DevProblem::cap_kind, f_alias
  int *u_f_alias = nullptr;
  std::vector<unsigned char> f_own;   // several ranks: DevProblem::f_own
  std::vector<int> big_caps;   // captures with more than kSchurMfmaBlocks distinct tags (k_schur's second launch)
  std::vector<int> chunk_caps;   // captures with more than kObsChunk observations (the chunked launches)
  int *u_chunk_caps = nullptr;
  unsigned char *u_obs_active = nullptr, *u_slot_free = nullptr;
  double *u_corners = nullptr, *u_x0 = nullptr;
  unsigned char *u_loss_kind = nullptr;   // DevProblem::obs_loss_kind, obs_loss_a (a problem with losses)
  double *u_loss_a = nullptr;
  double *u_obs_size = nullptr;           // DevProblem::obs_size (a problem with a tag side other than the default)
  long *u_cap_off = nullptr;
  int2 *u_dest_row = nullptr;
  int4 *u_gather_items = nullptr, *u_gather_splits = nullptr;
  arslam::SchurContrib *u_contrib = nullptr;
  // One rank, persistent executor: the fill tiles (numbered after the
  // assembled ones) are never cleared -- their first update stores.  n_clear:
  // the tiles k_schur clears (the assembled ones; every tile when an appended
  // problem's gather writes into a fill tile: then no first-update store)
  long n_clear = 0;
  DevBuf<double> d_xa, d_xb, d_xbest, d_g, d_colnorm, d_scale, d_diag;
  DevBuf<double> d_obs_tg, d_parts, d_fparts, d_red, d_S, d_z, d_yF;
  // the reduced system's tiles: Sp = d_S.p + s_pre.  Several ranks: the top
  // tags' linearization sums (top_tail_len doubles) ride in the prefix, just in
  // front of the top tiles, in the step's one bulk all-reduce
  double *Sp = nullptr;
  long s_pre = 0;
  int *u_top_slots = nullptr;
  int n_top_slots = 0;
  long top_tail_len() const { return 2L * n_top_slots + 2; }
  double *d_norms_p = nullptr;   // inside d_red
  DevBuf<int> d_flag;
  DevBuf<double> d_slab, d_jrows, d_cap_ui;
  DevBuf<double> d_gather_part;
  arslam::LltPlan plan;
  // x: the current point, xc: the candidate, xbest: the best point so far --
  // three of d_xa / d_xb / d_xbest by pointer, xc never aliasing the other two
  double *x = nullptr, *xc = nullptr, *xbest = nullptr;
  unsigned long long dbg_indefinite_mask = 0;   // arslam_lm_debug_force_indefinite
  arslam_iteration_callback iter_cb = nullptr;  // arslam_lm_set_iteration_callback
  void *iter_cb_ctx = nullptr;
  int n_fparts = 0;

  Timer timers[PH_N];
  arslam::LaunchTiming upd_timing;
  std::vector<hipEvent_t> upd_events;
  double dom_ms = 0.0, dom_flops = 0.0;
  double scalar_flops = 0.0;   // scalar Cholesky flops of the reduced system's real rows (ReducedLayout)
  long dom_launches = 0;

  void timing_begin();
  void timing_collect();   // after a stream synchronize

  // ---- multi-GPU ----
  int rank = 0, nranks = 1;
  ncclComm_t comm = nullptr;
  // debug (arslam_debug_force_multirank): take the multi-rank path -- the
  // split, the two-phase factorization and every collective -- with one rank,
  // so its RCCL calls run on a one-GPU box
  bool force_multi = false;
  bool multi() const { return nranks > 1 || force_multi; }

  ~arslam_lm();

  // host-callback transport (arslam_lm_set_comm_callback): stage through host memory
  arslam_allreduce_fn comm_cb = nullptr;
  void *comm_cb_ctx = nullptr;
  std::vector<unsigned char> comm_stage;

  // In-place all-reduce of a device buffer over the ranks (RCCL, or the
  // caller's callback).  Every rank issues the same sequence of calls.
  void allreduce_any(void *buf, size_t count, int dtype, int op);
  void allreduce(double *buf, size_t count, int op) { allreduce_any(buf, count, ARSLAM_DT_F64, op); }

  // Every rank derives the split itself (no structure is exchanged), so ranks
  // that disagree -- a rank-dependent environment, a different problem --
  // would issue mismatched collectives and hang.  One all-reduce (MAX of h and
  // of -h, 52-bit hash of the owner maps) proves they agree before the first step.
  DevBuf<double> d_split_hash;
  void check_same_split(const arslam::RankSplit &sp);

  int dag_workgroups = 512;
  const DebugEnv &env = debug_env();

  int cus_device = -1, cus = 0;   // the CU count, queried once per device
  // The thread and options device the handle's stream was last made ready
  // for: a later load from the same thread with the same options, while the
  // thread's current device is still the handle's, makes one hipGetDevice (a
  // thread-local read) and nothing else.  The current-device check matters
  // when one thread drives handles on several devices: another handle's load
  // may have switched it, and this handle's allocations must land on its own
  // device.
  std::thread::id ready_thread{};
  int ready_opt_device = -2;
  void ensure_stream();

  // (in_loss, here and in try_append: the losses of p's observations, in p's
  // order, null arrays for none; they go beside the corners into every
  // host_problem call of the load)
  void load(const arslam_soa_problem *p, const arslam::ObsLoss &in_loss);
  // load()'s stages: the e-block side for Ceres' set cs and the device problem
  // of that side; several ranks: this rank's problem h, the whole problem's
  // layout L (for the order memory's request rq), this rank's column classes;
  // the tile plan (+ one rank: the gather plan and the order's graph); the timings
  int choose_side(const arslam::SchurSide &cs);
  const arslam_soa_problem *choose_device_problem(const arslam_soa_problem *p_in, arslam_soa_problem &swapped);
  void local_rank_problem(const arslam_soa_problem *p, const arslam::ObsLoss &in_loss, const arslam::LayoutRequest &rq,
                          arslam::HostProblem &h, arslam::ReducedLayout &L, std::vector<int> &col_class);
  void build_plans(const arslam::HostProblem &h, arslam::ReducedLayout &L, const std::vector<int> &col_class);
  void record_load_times(double t_load, double t_side, double t_host, double t_layout, double t_book, double t_plan,
                         double t_upload);
  // (extend_from >= 0: captures [extend_from, nc) were appended to the loaded
  // problem, the others unchanged: the gather plan is extended, not rebuilt)
  void upload_problem(const arslam::HostProblem &h, const arslam::ReducedLayout &L, int extend_from = -1);
  void alloc_solve_buffers();   // (upload_problem's: after the gather plan and the tile plan)
  arslam::SchurGather sg;   // the loaded problem's Schur gather plan
  bool sg_ready = false;    // load(): sg was built beside the tile plan (upload_problem keeps it)
  // the append path (lm_load.hip): one entry, a front end per eliminated side, shared checks
  bool try_append(const arslam_soa_problem *p, const arslam::ObsLoss &in_loss);
  bool append_as_captures(const arslam_soa_problem *p);
  bool append_as_mixed(const arslam_soa_problem *p, arslam::MixedProblem &m);
  bool same_reduced_rows(const arslam::HostProblem &h) const;
  bool groups_fit_plan(const arslam::HostProblem &h, const std::vector<int> &groups) const;
  arslam::ReducedLayout lay;      // the loaded layout (one rank), kept for try_append
  bool pk_appended_only = false;  // since the last load only residual blocks of known tags were added
  int setup_kind = ARSLAM_SETUP_LOAD;
  int elim_used = ARSLAM_ELIM_CAPTURES;   // the side load() eliminates (the device problem is role-swapped for TAGS)
  arslam::MixedProblem mx;                // ARSLAM_ELIM_MIXED: the regrouped device problem (host_structure.h)
  int ceres_e_cap = 0, ceres_e_tag = 0;   // Ceres 2.0's e-block set of the loaded problem, by kind
  void reload_values(const arslam_soa_problem *p);
  bool pk_loaded = false;   // the resident problem came from the pointer-keyed API
  // several ranks: the whole problem's capture count, this rank's captures
  // (ascending; the loaded problem's capture c is own_caps[c]) and its local arrays
  int nc_full = 0;
  int nc_user = 0;   // the caller's capture count (the device problem's "captures" are tags or groups under TAGS / MIXED)
  std::vector<int> own_caps;
  std::vector<double> loc_cap, loc_corners;
  std::vector<int> loc_obs_cap, loc_obs_tag;
  std::vector<unsigned char> loc_cap_const;
  std::vector<unsigned char> loc_loss_kind;   // this rank's observations' losses
  std::vector<double> loc_loss_a;
  std::vector<double> loc_size;               // ... and their tags' sides
  double split_top_work = 0.0, split_max_rank_work = 0.0, split_total_work = 0.0;
  int split_active = 1;   // ranks owning subtrees (RankSplit::n_active)
  // the elimination order kept between loads, and the pointer-keyed path's
  // request to keep it (set around its load() of a grown problem)
  arslam::OrderMemory order;
  bool reuse_order = false;
  void linearize(double *x_cost, double *fixed_cost, double *gmax, double *gnorm, double *xnorm);
  // linearize split at the host read: enqueue (results copied to h_lin), collect after a sync
  void linearize_launch();
  void linearize_collect(double *x_cost, double *fixed_cost, double *gmax, double *gnorm, double *xnorm);
  // Several ranks: a linearization's sums over the ranks are not collectives
  // of their own.  Its tag slots' gradient and column norms and the camera's
  // f partials (lin_xpending) ride in front of the top tiles in the next
  // step's bulk all-reduce (or one packed all-reduce, complete_pending_lin,
  // when no step follows); its cost and norms (norms_pending) ride with the
  // step's scalars (exchange_scalars; exchange_norms when no step follows).
  bool lin_xpending = false, norms_pending = false;
  DevBuf<double> d_lx, d_ag;   // the packed exchange; the all-gathered scalars
  static constexpr int kLinSave = 16 + 8 + 6 * arslam::kNormBlocks;   // d_red[kLinSave..+1]: the linearization's cost, fixed
  void complete_pending_lin();
  void lin_norms();   // k_slot_norms once the linearization's sums are final
  void exchange_scalars(arslam::AgFields fl, arslam::HostOut *ho = nullptr);   // (+ the pending norms), into d_red
  void exchange_norms() {
    if (norms_pending) exchange_scalars(arslam::AgFields{});
  }
  PinnedBuf h_lin;   // [0..3] cost, fixed, g_f, col_f; [16..21] slot norms; [16 + kHostSeq] lin_seq
  double lin_seq = 0.0;   // (one rank) the last linearization's sequence number
  void lin_sync() {   // the linearization's host words (one rank: its flag; several: after the copies)
    if (!multi() && lin_seq > 0.0) flag_sync(h_lin.p + 16 + arslam::kHostSeq, lin_seq);
    else spin_sync();
  }
  // host LM loop: the Jacobi scale of this solve is set, so each later
  // linearization also forms the LM diagonal (k_slot_norms) and the step's
  // executor reset rides in k_schur's launch
  bool diag_in_lin = false;
  PinnedBuf h_x;     // [n] parameter download (write_back)
  PinnedBuf h_step;  // [0..NPART+1] the step's reduced scalars, [NPART+2..4] the factorization flags
  hipEvent_t ev_sync = nullptr;
  // Wait for the stream by polling an event: the LM loop's one host round
  // trip per step, without the blocking-sync wake-up latency.
  void spin_sync() {
    if (!ev_sync) HIP_CHECK(hipEventCreateWithFlags(&ev_sync, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(ev_sync, stream));
    hipError_t e;
    while ((e = hipEventQuery(ev_sync)) == hipErrorNotReady) {
    }
    HIP_CHECK(e);
  }
  // One rank: the LM loop's host reads wait for the kernel that stores their
  // page-locked words to store its sequence number last (hout[kHostSeq]),
  // instead of an event behind it: ~8 against ~13 us per round trip on
  // MI355X (tools/sync_bench.hip), ~7 round trips per cfg3 solve and ~7,000
  // in the incremental cfg2 flow.  The stream is queried now and then so a
  // launch that never stores it (an error) is reported, not waited for.
  double host_seq = 0.0;
  DevBuf<int> d_seq_done;   // k_reduce_parts' finished blocks (zero between launches)
  double next_seq(double *word) {
    *(volatile double *)word = -1.0;   // (before the launch: the kernel's store lands after it)
    return host_seq += 1.0;
  }
  void flag_sync(const double *word, double seq) {
    for (long k = 1;; ++k) {
      if (*(const volatile double *)word == seq) break;
      if ((k & 4095) == 0) {
        const hipError_t e = hipStreamQuery(stream);
        if (e == hipErrorNotReady) continue;
        HIP_CHECK(e);
        if (*(const volatile double *)word == seq) break;
        throw Error(ARSLAM_E_DEVICE, "the stream finished without storing the host sequence word");
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  // solve() is the trust-region loop; its stages are plain members (lm_solve.hip)
  void solve(arslam_lm_summary *s);
  void begin_solve(arslam_lm_summary *s);
  // one step's launches: returns the sequence number h_step will hold (solve_index: from 0)
  double enqueue_step(double radius, bool reuse_diag, int solve_index);
  bool prepare_step(bool reuse_diag, arslam::ExecReset *er);   // true: the executor reset rides in k_schur (er)
  // The one place that factors the reduced system Sp of the loaded plan with
  // opt.factor_executor.  first_store: launch_dense_llt_dag's bound; record:
  // kernel timing (after timing_begin); radius, force_indefinite: several ranks
  // only (the top rows' D^2 and the test hook, between the two phases)
  void factor_reduced(long first_store, bool record, double radius = 0.0, bool force_indefinite = false);
  void dump_dag_trace(long first_store);   // ARSLAM_DAG_TRACE: a stamped launch and its file
  void back_substitute(double radius);
  double reduce_step_scalars();
  void fill_summary(arslam_lm_summary *s);
  void write_back(const double *d_src);
  // the pointer-keyed solve in progress: its (unswapped) staging problem, whose
  // arrays soa aliases; write_back also scatters them into the caller's blocks
  const arslam_soa_problem *pk_stage = nullptr;
  void scatter_to_blocks();
  // arslam_lm_debug_break_dependency: the patched wait entry, restored after the next solve
  int dbg_patched_wait = -1;
  void restore_patched_wait();
  // multi-rank: does any rank have an iteration callback (agreed once per solve)
  bool any_iter_cb = false;
  DevBuf<double> d_cb;
  int agree_callback(int r);

  // ---- marginal covariances (arslam_lm_covariance) ----
  // the last solve of the loaded problem: 0 none completed, 1 completed, 2 ended with EVAL_FAILED
  int solve_state = 0;
  // everything below is allocated at the first covariance call
  arslam::SelinvPlan cov_sp;
  bool cov_sp_ready = false;   // cov_sp is the loaded plan's
  DevBuf<double> d_cov_Z, d_cov_Q, d_cov_Y, d_cov_R, d_cov_out, d_cov_diag;   // d_cov_out: e-blocks 36 nc | f-blocks 36 nt | var(f)
  // the e-blocks' G_la = Q'L_a, 12 each: allocated at the first _lens call on a
  // problem whose l1, l2 are live (d_cov_out then ends with the camera's 3x3)
  DevBuf<double> d_cov_Gl;
  DevBuf<int> d_cov_status;
  hipEvent_t cov_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  // The anchored forms (arslam_lm_covariance_anchored): the pose block held
  // fixed for one call besides the constant ones (kind ARSLAM_BLOCK_CAPTURE,
  // _TAG or _NONE, the caller's index).
  struct CovAnchor {
    int kind = ARSLAM_BLOCK_NONE, index = 0;
    bool none() const { return kind == ARSLAM_BLOCK_NONE; }
    bool operator==(const CovAnchor &o) const { return kind == o.kind && (none() || index == o.index); }
  };
  // The form of a covariance call and of the kept result: plain, _lens (the
  // camera's block is [f, l1, l2]) or _anchored (a _lens form with an anchor,
  // possibly NONE; it takes the mixed e-block set too).  Equal forms serve each
  // other's kept result: plain only plain, lens only lens, anchored the same anchor.
  struct CovForm {
    bool lens = false, anchored = false;
    CovAnchor anchor{};
    static CovForm with_lens() { return CovForm{true, false, CovAnchor{}}; }
    static CovForm anchored_at(const CovAnchor &an) { return CovForm{true, true, an}; }
    bool operator==(const CovForm &o) const {
      return lens == o.lens && anchored == o.anchored && (!anchored || anchor == o.anchor);
    }
    // the entry point of this form in messages: "covariance" -> "covariance_lens", ...
    std::string name(const char *stem) const { return std::string(stem) + (anchored ? "_anchored" : lens ? "_lens" : ""); }
  };
  // the kept result of covariance(), in the caller's block order, and the form
  // it was computed for (the pointer-keyed block forms serve it to that form alone)
  bool cov_kept = false;
  CovForm cov_form{};
  std::vector<double> cov_cap, cov_tag;
  std::vector<int> cov_cap_status, cov_tag_status;
  double cov_var_f = -1.0;
  double cov_cam[9] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};   // the camera's 3x3 over [f, l1, l2] and its status
  int cov_cam_status = ARSLAM_COV_UNAVAILABLE;
  arslam_lm_cov_info cov_info{};
  // allocated at the first anchored call: the call's copy of the Jacobi scale
  // (0 on the anchor's slots and on the direct groups' copies) and, under a
  // mixed e-block set, its direct groups
  DevBuf<double> d_cov_scale;
  DevBuf<int> d_cov_direct;
  void covariance(const CovForm &form);
  void cov_invalidate() {
    solve_state = 0;
    cov_kept = false;
  }
  // The one map between the caller's blocks and the device problem's: per
  // capture and tag the role (arslam::kCovE: a group's eliminated block, kCovF:
  // an f-block) and the index there, from elim_used (whole sides) or mx (a mixed
  // set: kind, group_src, f_src, f_is_cap); a reduced capture is kCovF.  e_node /
  // f_node: the caller's block (capture c: c, tag t: n_cap + t) of each group and
  // f-block -- a direct group's is its capture's, the block its f-block is.
  // Derived per call (block_map), never kept: load and try_append change it.
  struct BlockMap {
    int n_cap = 0, n_tag = 0;
    std::vector<int> cap_role, cap_idx, tag_role, tag_idx;
    std::vector<int> e_node, f_node;
    int role(bool cap, int i) const { return cap ? cap_role[i] : tag_role[i]; }
    int idx(bool cap, int i) const { return cap ? cap_idx[i] : tag_idx[i]; }
    // the device problem's block (e-blocks, then f-blocks) of a caller's block; -1: none
    long device_block(bool cap, int i, int nc) const {
      return idx(cap, i) < 0 ? -1 : role(cap, i) == arslam::kCovE ? idx(cap, i) : (long)nc + idx(cap, i);
    }
  };
  BlockMap block_map() const;
  // the form's anchor as the calls accept it (throws ARSLAM_E_INVALID_ARG otherwise)
  void cov_check_anchor(const std::string &who, const CovForm &form, const BlockMap &bm) const;
  // What covariance() and covariance_pairs() share (lm_covariance.hip):
  // cov_check_state: the calls' preconditions.  cov_factor: the device
  // problem's structure read back, the structural gauge check on the host, then
  // -- unless it fails -- the linearization at xbest, k_cov_schur, the gather
  // with the covariance's diagonal and the factorization, all enqueued
  // (cov_ev[0..2] around them); S then holds the factor itself.
  // cov_numeric_test: after the caller's own launches, the one stream sync, the
  // flag and the min_pivot test; fills the times.
  struct CovFactor {
    std::vector<int> cap_start;   // the device problem's e-block CSR
    bool deficient = false;
    bool factored = false;        // the device work was enqueued
    bool live = false;            // a _lens call on a problem whose l1, l2 are estimated: they are rows of H
    arslam_lm_cov_info info{};
    // the Jacobi scale every covariance kernel of the call reads: the handle's,
    // or an anchored call's copy (d_cov_scale)
    const double *scale = nullptr;
    // an anchored call's anchor in the device problem: its role, index and
    // first slot; role -1: none
    int anchor_role = -1, anchor_idx = -1;
    long anchor_slot = -1;
    bool is_anchor(int role, int idx) const { return anchor_role >= 0 && role == anchor_role && idx == anchor_idx; }
  };
  bool cov_e_free(int c) const { return slot_free[3 + 6L * c] != 0; }
  bool cov_f_free(int t) const { return slot_free[3 + 6L * nc + 6L * t] != 0; }
  void cov_check_state(const std::string &who, const CovForm &form) const;
  // cov_factor's stages: what it reads back of the device problem (and, for an
  // anchored form, of the Jacobi scale), and the enqueue after the gauge check
  struct CovStructure;
  void cov_read_structure(CovFactor &cf, const CovForm &form, CovStructure &st);
  void cov_enqueue(CovFactor &cf, const CovForm &form, CovStructure &st, bool assemble_only);
  void cov_factor(CovFactor &cf, const CovForm &form, const BlockMap &bm, bool assemble_only = false);
  void cov_numeric_test(CovFactor &cf);

  // ---- cross-covariance blocks (arslam_lm_covariance_pairs) ----
  // everything below is allocated at the first covariance_pairs call
  arslam::TileSolvePlan cov_tp;
  bool cov_tp_ready = false;   // cov_tp is the loaded plan's
  static constexpr int kCovBatchPanels = 16;              // panels solved per batch at most (160 right-hand blocks) ...
  static constexpr size_t kCovBatchBytes = 256u << 20;   // ... within this many bytes of panels, one panel at least
  DevBuf<unsigned char> d_pair_mask;   // per panel: active tile rows, then needed tile rows
  DevBuf<double> d_pair_B, d_pair_out;
  DevBuf<int2> d_pair_rhs;
  DevBuf<arslam::CovPairTask> d_pair_tasks;
  DevBuf<int> d_pair_status;
  std::vector<hipEvent_t> pair_ev;   // two per batch, around its solve
  void covariance_pairs(const CovForm &form, const arslam_lm_cov_pair *pairs, int n_pairs, double *cov, int *status,
                        arslam_lm_cov_info *info);
  // its plan (the pairs resolved, the distinct tasks; host functions of
  // lm_covariance.hip fill it) and the two stages that use the device
  struct CovPairPlan;
  void cov_pair_masks(const CovFactor &cf, CovPairPlan &pp);
  void cov_pair_batches(CovFactor &cf, CovPairPlan &pp);

  // ---- Evaluate (arslam_lm_evaluate*, lm_evaluate.hip) ----
  // A path of its own: the problem's structure in the caller's order, its own
  // buffers, nothing of the solver's device state.  Everything below is
  // allocated and uploaded at the first evaluate after a load or an added block.
  // the problem arslam_lm_load_soa* was given, in the caller's roles (load()'s
  // soa is the device problem's), and its explicit per-observation losses (the
  // default loss's are soa_loss_*, the sides soa_size)
  arslam_soa_problem ev_src{};
  bool ev_src_set = false, ev_src_sized = false;
  int ev_src_loss_from = 0;   // 0 no loss, 1 ev_src_kind / ev_src_a, 2 soa_loss_kind / soa_loss_a
  std::vector<unsigned char> ev_src_kind;
  std::vector<double> ev_src_a;
  // the device structure (pointers into ev_upload) and what it was built for
  bool ev_valid = false, ev_pk = false;
  int ev_nc = 0, ev_nt = 0, ev_nb = 0, ev_mode = 0;   // ev_mode: 0 pinhole, 1 radial held, 2 radial estimated
  bool ev_loss = false, ev_sized = false, ev_cam_const = false;
  UploadArena ev_upload;
  arslam::EvalProblem EV{};
  DevBuf<double> d_ev_x, d_ev_res, d_ev_obs, d_ev_parts, d_ev_out;
  PinnedBuf h_ev_x;
  // options.phase_timing: the last evaluate's upload, k_eval_obs, k_eval_blocks,
  // k_eval_tree (both launches) and copy back, ms (arslam_lm_debug_evaluate_times)
  hipEvent_t ev_evt[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double ev_ms[5] = {0, 0, 0, 0, 0};
  bool ev_ms_valid = false;
  // the last arslam_lm_evaluate_blocks' gradient (arslam_lm_gradient_block)
  bool ev_grad_valid = false;
  std::vector<double> ev_grad;
  // whatever drops the loaded problem or changes the blocks drops the structure
  void eval_drop() {
    ev_valid = false;
    ev_grad_valid = false;
  }
  void eval_upload_structure(bool pk);
  void evaluate(bool pk, const arslam_lm_evaluate_options *opt, double *cost, double *residuals, double *sq_norm,
                double *weight, double *gradient);
};
