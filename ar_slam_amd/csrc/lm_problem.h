// lm_problem.h -- the device problem of the LM solver: the constants of its
// row and LDS layouts, the per-capture partial sums (PartIdx), `DevProblem`
// (every device array a kernel reads about the loaded problem) and the
// addressing of the compact-tiled reduced system.  Shared by the LM driver
// (lm_handle.h), the LM stages' kernels (lm_linearize.hip, lm_schur.hip,
// lm_step.hip, lm_reduce.hip, lm_exchange.hip) and the covariance kernels
// (selinv.hip, cov_pairs.hip).
//
// Parameter slots (one contiguous f64 vector, x):
//   [0,3)                camera  f, l1, l2
//   [3 + 6c, 9 + 6c)     capture c inv_pose  t_c, w_c
//   [3 + 6Nc + 6t, ...)  tag t pose  t_t, w_t
// Reduced (f-side) rows: tag t -> tag_row[t] + a, camera -> cam_row + b, in an
// ordering chosen on the host (llt_plan.cpp); the camera comes last, so the
// reduced matrix is an arrow-head (sparse tag block + one dense border).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

#include "host_structure.h"

namespace arslam {
constexpr int kWave = 64;
constexpr int kTile = 64;          // reduced-system Cholesky tile
constexpr int kRowStride = 14;     // LDS row: 13 Jacobian entries + residual
// The stored copy of a row (DevProblem::jrows): 11 values.  The capture- and
// tag-translation columns of a row are the same three numbers (d/dt_c =
// d/dt_t = P M_c: the point is R_t corner + t_t + t_c), so columns 7..9 are
// not stored; column j of the row is stored column jrow_col(j).
constexpr int kJStored = 11;
__host__ __device__ constexpr int jrow_col(int j) {
  return j <= 6 ? j : j <= 9 ? j - 6 : j <= 12 ? j - 3 : 10;
}
// The per-capture kernels take a capture's observations through LDS in
// chunks of kObsChunk (8 observations = one wave's 64 residual rows), so
// k_linearize, k_backsub and the cost take any number of observations per
// capture.  k_schur keeps the capture's local system over its distinct tags
// in LDS: up to kSchurMfmaBlocks tags (m + 1 <= 64 local rows) it forms it as
// one MFMA product in the main launch; captures with more tags run in a second
// launch sized for them, up to kMaxSchurBlocks distinct tags (its LDS at
// schur_lds_bytes(kMaxSchurBlocks) <= 160 KiB, the CU's LDS).
constexpr int kObsChunk = 8;
constexpr int kSchurMfmaBlocks = 10;
// k_schur's dynamic LDS for captures of at most nblk distinct tags (the
// layout at the top of k_schur)
constexpr size_t schur_lds_bytes(int nblk) {
  // stage 6 min(m + 1, 64) | tscale 6 kObsChunk | U 36 | Ui 36 | Etr 8 | W 6 m | Ftr m (+1) | FF 28 nblk |
  // lblk (ints, kObsChunk + 2) | ff00
  return sizeof(double) * (6 * ((6 * nblk + 2) < 64 ? (6 * nblk + 2) : 64) + 6 * kObsChunk + 36 + 36 + 8 +
                           7 * (6 * nblk + 1) + 2 + 28 * nblk) +
         sizeof(int) * (kObsChunk + 2) + 2 * sizeof(double) + 64;
}
static_assert(schur_lds_bytes(kMaxSchurBlocks) <= 160 * 1024, "k_schur's LDS at kMaxSchurBlocks");
// That layout's arrays as indices of doubles from the start of the wave's LDS
// (stage is at 0), for a capture of nblk distinct tags: k_schur's pointers and
// the LDS indices in its output stage's descriptor table (schur_store_table.h)
struct SchurLds {
  int tscale, U, Ui, Etr, W, Ftr, FF, lblk, ff00;
};
__host__ __device__ constexpr SchurLds schur_lds(int nblk) {
  const int m = 1 + 6 * nblk;
  SchurLds l{};
  l.tscale = 6 * (m + 1 < kWave ? m + 1 : kWave);
  l.U = l.tscale + 6 * kObsChunk;
  l.Ui = l.U + 36;
  l.Etr = l.Ui + 36;
  l.W = l.Etr + 8;
  l.Ftr = l.W + 6 * m;
  l.FF = l.Ftr + m + (m & 1);
  l.lblk = l.FF + 28 * nblk;            // kObsChunk ints
  l.ff00 = l.lblk + kObsChunk / 2;
  return l;
}

// number of per-capture partial sums written by the per-capture kernels
enum PartIdx {
  P_COST = 0,        // sum 0.5|r|^2 over active observations
  P_FIXED = 1,       // same, observations whose blocks are all constant
  P_GF = 2,          // camera-f gradient partial
  P_CF = 3,          // camera-f squared column norm partial
  P_MODEL = 4,       // model cost change partial  p.(r - p/2)
  P_STEP2 = 5,       // squared step norm (capture slots)
  P_YBAD = 6,        // non-finite step flag (max)
  P_CBAD = 7,        // non-finite candidate residual flag (max)
  NPART = 8
};

struct DevProblem {
  int nc, nt, nb;
  // 1: loaded under ARSLAM_CAMERA_RADIAL -- the host then launches the kDist
  // instances of k_linearize, k_cost and k_backsub, which read l1 and l2 from
  // camera slots 1 and 2; no kernel reads the flag.  (In the four bytes that
  // padded nb up to n: no field's kernel-argument offset moves.)
  int camera_radial = 0;
  long n;              // number of parameter slots 3 + 6nc + 6nt
  long nR;             // rows of the reduced system (tags + camera + alignment padding); row nR = rhs
  long N;              // padded matrix size (multiple of kTile, > nR)
  long lda;            // leading dimension of S
  int max_obs_per_cap;
  int max_blk_per_cap;       // most distinct tags (f-blocks) of one capture
  // captures with more than kSchurMfmaBlocks distinct tags (k_schur's second
  // launch); null when there are none
  const int *big_caps = nullptr;
  int n_big_caps = 0;
  // captures with more than kObsChunk observations (the chunked launches of
  // k_linearize, k_cost and k_backsub); null when there are none
  const int *chunk_caps = nullptr;
  int n_chunk_caps = 0;
  // 1: the e-blocks (the "capture" slots, CSR cap_start) are the problem's tags
  // and the f-blocks (the "tag" slots) its captures -- ARSLAM_ELIM_TAGS: the
  // residual is then evaluated with the two pose arguments exchanged and the
  // two 6-column halves of its Jacobian row swapped back into e|f order
  int swap_roles;
  // ARSLAM_ELIM_MIXED (MixedProblem): each group's kind (kMixCap, kMixTag --
  // roles swapped for that group -- or kMixDirect), and per f-block the direct
  // group whose slot copies it, -1; null otherwise (swap_roles holds for all)
  const unsigned char *cap_kind = nullptr;
  const int *f_alias = nullptr;
  int nf;                    // f-side parameter slots: camera 3 + 6 nt
  const int *fslot_row;      // [nf]    reduced row of f-side slot j (camera j < 3, tag slot 3 + 6 t + a), -1 if none
  int cam_row;               // first reduced row of the camera block, -1 if the camera is not free
  const int *cap_start;      // [nc+1]  CSR of observations by capture
  const int *obs_tag;        // [nb]
  const int *obs_lblk;       // [nb]    local f-block (1..) of the observation's tag in its capture
  const int *cap_blk_start;  // [nc+1]  CSR of distinct tags per capture
  const int *blk_tag;        // [sum]   tag of each local block
  const unsigned char *obs_active;   // [nb]
  const unsigned char *slot_free;    // [n]
  const int *tag_start;      // [nt+1]  CSR of observations by tag (capture-major order inside)
  const int *obs_tpos;       // [nb]    position of each observation in that CSR: k_linearize's per-observation
                             //         tag sums are stored tag-major (obs_tg), so a tag's are contiguous
  const double *corners;     // [nb*8]
  const int *tag_row;        // [nt]    first reduced row of tag t (6 rows), -1 if not free
  const int *row_slot;       // [nR]    parameter slot of a reduced row, -1 for padding rows
  const int *tile_id;        // [T*T]   compact tile index of the reduced system (see LltPlan)
  int T;                     // tiles per side
  // deterministic Schur assembly (SchurGather): packed local systems + gather lists
  const long *cap_off;       // [nc+1]
  double *slab;              // [cap_off[nc]]
  const int2 *dest_row;      // [n_dest] first rows (rX, rY) of each destination block
  const int *dest_start;     // [n_dest+1]
  const SchurContrib *contrib;
  int n_dest;
  const int4 *gather_items;  // [n_items] {destination, first, end contribution, partial slot or -1}
  const int4 *gather_splits; // [n_splits] {destination, first partial slot, pieces, 0}
  double *gather_part;       // [n_pslots * 36]
  int n_items, n_splits;
  // multi-rank: class of each tile column (0 this rank's subtree, 1 the
  // replicated top, 2 another rank's; LltPlan::tile_class), null on one rank
  const signed char *tile_class;
  // several ranks: the f-side slots whose values this rank holds (its own
  // subtree's tags; the replicated top's tags, the camera and the constant
  // tags on rank 0 only), null on one rank: the sums over f-side slots
  // (x^2, the f-side step) count each slot on one rank, and the final tag
  // values are gathered from these
  const unsigned char *f_own = nullptr;
  double *jrows;             // [8 nb kJStored] unscaled Jacobian rows + residual at the linearization point
                             // (an observation with a loss: its rows times sqrt(rho'), Ceres' corrector)
                             // (column-major per capture: (row, jrow_col(j)) at 8 o0 kJStored + jrow_col(j) 8k + row)
  double *cap_ui;            // [36 nc] (U_c + D_c^2)^{-1} of the current step (k_schur -> k_backsub)
  // the observations' robust losses (loss.h), in the order of corners; both
  // null when no observation of the loaded problem has one -- the host then
  // launches the kLoss = false instances of k_linearize, k_cost and k_backsub
  // (last in the struct: no other field's kernel-argument offset moves)
  const unsigned char *obs_loss_kind = nullptr;   // [nb] ARSLAM_LOSS_*
  const double *obs_loss_a = nullptr;             // [nb] scale a
  // the side length of each observation's tag, in the order of corners; null
  // when every tag of the loaded problem has the default side -- the host then
  // launches the kSized = false instances (per observation, not per tag: the
  // groups of swap_roles and the mixed e-set need no tag lookup)
  const double *obs_size = nullptr;               // [nb] metres
};

// The handle's "estimate the distortion" switch on a problem loaded under
// ARSLAM_CAMERA_RADIAL with a free camera: what the kernels of that path read
// and write besides DevProblem.  A struct of its own, passed to those kernels
// alone: DevProblem and every kernel that takes it stay as they are.
// jrows_l: the rows' two l columns beside jrows ((row, a) of a capture at
// 16 o0 + a 8k + row).  lparts, lred: k_linearize_est's per-capture partials of
// the l gradient and squared column norms and their sums.  cam_slab:
// k_schur_cam's border of the Schur complement, 2 (m + 3) values per e-block c
// (m = 1 + 6 distinct f-blocks) at 8 c + 12 cap_blk_start[c]: for a in
// {l1, l2} the entries against f, the local tag columns, l1, l2 (b <= a) and
// the rhs.  camg_*: per f-block the (e-block, local block) pairs that see it,
// in e-block order (the border gather's summation order).
struct DevCamL {
  double *jrows_l = nullptr;        // [16 nb]
  double *lparts = nullptr;         // [4 nc]
  double *lred = nullptr;           // [4]
  double *cam_slab = nullptr;       // [8 nc + 12 cap_blk_start[nc]]
  const int *camg_start = nullptr;  // [nt + 1]
  const int2 *camg_items = nullptr; // [cap_blk_start[nc]] {e-block, local block 0..}
};

// where e-block c's border lives in DevCamL::cam_slab, and its leading dimension m + 3
__device__ __forceinline__ long cam_slab_off(const DevProblem &P, int c) { return 8L * c + 12L * P.cap_blk_start[c]; }
__device__ __forceinline__ int cam_slab_ld(const DevProblem &P, int c) {
  return 4 + 6 * (P.cap_blk_start[c + 1] - P.cap_blk_start[c]);
}

// element (r, c), r >= c, of the compact-tiled reduced system
__device__ inline double *reduced_elem(double *S, const DevProblem &P, long r, long c) {
  return S + (long)P.tile_id[(r >> 6) * P.T + (c >> 6)] * 4096 + (r & 63) * 64 + (c & 63);
}

}  // namespace arslam
