// lm_cov.h -- the covariance of the LM solver on the device: the selected
// inverse of the factored reduced system and the marginal blocks (selinv.hip),
// the multi-right-hand-side tile solve and the cross-covariance blocks
// (cov_pairs.hip), and the border and block kernels of a problem whose l1, l2
// are estimated (cov_lens.hip), and the local systems of a mixed e-block
// set's direct groups (cov_direct.hip).  Called by lm_covariance.hip (the
// entry points, lm_cov_capi.hip, launch nothing), and by debug_tiles.hip for
// the component tests.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>

#include "llt_plan.h"
#include "lm_problem.h"

namespace arslam {

// ---- selinv.hip ----
// Selected inverse of the factored reduced system on the factor's tile
// pattern (one-rank plans).  gcol[g]: the position in bs_cols of gather g's
// column; n_products: its 64x64x64 tile products.
struct SelinvPlan {
  int *gcol = nullptr;
  long n_products = 0;
};
void selinv_plan_build(const LltPlan &P, SelinvPlan &sp, hipStream_t s);
void selinv_plan_free(SelinvPlan &sp);
// After a factorization of S (launch_dense_llt or launch_dense_llt_dag): Z =
// the real rows' (< nR) inverse on the plan's tiles (P.n_tiles x 4096, tile_id
// addressing; diagonal tiles full and exactly symmetric, off-diagonal tiles
// (i, k), i > k).  Overwrites the off-diagonal tiles of S.  Level launches on s.
void launch_selinv(const LltPlan &P, const SelinvPlan &sp, double *S, long nR, double *Z, const int *flag,
                   hipStream_t s);
// The marginal 6x6 blocks of the covariance at the linearization in P.jrows,
// in the device problem's block order, unscaled by the Jacobi scale:
//   cov_f [36 nt], var_f [1]: the reduced-side blocks and the focal from Z (-1
//     where the block has no reduced row);
//   cov_e [36 nc], status_e [nc]: the eliminated blocks, R^{-1} (I + G Z G^T)
//     R^{-T} from launch_cov_schur's G and R (one wavefront each; status 0
//     computed, 1 constant or unused, 2 its R is singular; -1 in the block
//     unless 0).
// Z may be null when there is no reduced system.  *flag != 0: -1 everywhere.
void launch_cov_blocks(const DevProblem &P, const double *Z, const double *scale, const double *Gb, const double *Rb,
                       double *cov_e, int *status_e, double *cov_f, double *var_f, const int *flag, hipStream_t s);
// The covariance's elimination of every e-block from P.jrows by an orthogonal
// factorization E = Q R of its scaled columns (one wavefront each): G = Q'F
// and R are kept for launch_cov_blocks, and with write_slab the local reduced
// systems F'F - G'G go to P.slab in k_schur's layout (launch_schur_gather
// then assembles S).  Scratch: Qb 48 nb doubles, Gb 6 (nc + 6 sum of the
// e-blocks' distinct f-blocks), Rb 36 nc.
void launch_cov_schur(const DevProblem &P, const double *scale, double *Qb, double *Gb, double *Rb, bool write_slab,
                      hipStream_t s);

// ---- cov_pairs.hip ----
// Multi-right-hand-side solve X = L^{-T} L^{-1} B over the factor's tiles
// (one-rank plans).  The forward pass is left-looking: per backward column b
// (bs_cols order) the off-diagonal tiles (k, j) of tile row k = bs_cols[b],
// ascending j, as {j, tile id} in flist[fbeg[b] .. fbeg[b + 1]).
struct TileSolvePlan {
  int *fbeg = nullptr;
  int2 *flist = nullptr;
  std::vector<int> h_fbeg;     // host copies
  std::vector<int2> h_flist;
  std::vector<int> parent;     // [T] tile elimination tree: the first off-diagonal tile row of column k, -1 for a root
};
void tile_solve_plan_build(const LltPlan &P, TileSolvePlan &tp, hipStream_t s);
void tile_solve_plan_free(TileSolvePlan &tp);
// A panel's masks, [T] bytes each (both closed under the elimination tree's
// ancestors; tile_solve_mark closes them): active: the tile rows where the
// right-hand sides are non-zero -- the forward pass skips every other tile row
// and every product with an inactive Y_j, all exactly zero; needed: the tile
// rows of X somebody reads -- the backward pass computes those alone (a column
// reads its ancestors only).
void tile_solve_mark(const TileSolvePlan &tp, unsigned char *mask, long row);   // the tile of reduced row `row` and its ancestors
// 64x64x64 tile products of one panel's solve under its masks (null: none), the diagonal inverses included
long tile_solve_products(const LltPlan &P, const TileSolvePlan &tp, const unsigned char *active,
                         const unsigned char *needed);
// B: n_panels panels of 64 right-hand sides, each P.T row-major 64x64 tiles
// (tile row k of panel p at B + (p T + k) 4096), rows >= nR zero; solved in
// place against the factor in S (off-diagonal tiles) and P.ldiag, as
// launch_dense_llt / launch_dense_llt_dag leave them -- not after
// launch_selinv, which overwrites S.  Rows >= nR of X are zero.  active, needed:
// device masks [n_panels * P.T] as above, or null for a full solve (tile rows
// that are not needed keep their forward values).  Level launches on s; nothing
// is written when *flag != 0.
void launch_tile_solve(const LltPlan &P, const TileSolvePlan &tp, const double *S, long nR, double *B, int n_panels,
                       const unsigned char *active, const unsigned char *needed, const int *flag, hipStream_t s);
// A parameter block of the device problem: the focal, f-block idx (reduced
// side) or e-block idx (eliminated side).  A panel holds kCovPanelBlocks
// 6-column blocks and 4 zero columns, so no block straddles two panels.
enum { kCovFocal = 0, kCovF = 1, kCovE = 2 };
constexpr int kCovPanelBlocks = 10;
// The right-hand sides of rhs[0 .. n_rhs) ({role, idx}, device) into the
// zeroed panels B, block s in columns 6 (s % 10) .. of panel s / 10: unit
// columns for the focal (one) and an f-block, -(R^{-1} G)^T scattered for an
// e-block (from launch_cov_schur's G and R).
void launch_cov_pair_rhs(const DevProblem &P, const double *Gb, const double *Rb, const int2 *rhs, int n_rhs,
                         double *B, hipStream_t s);
// Block (a, b) of the covariance from the solved panels X, b the block whose
// columns sit in panel slot `slot`; 36 values (rows of a, columns of b; the
// focal has one row / column, the rest 0) to out + 36 `out`, and status[out]:
// 0 computed, 2 an e-block's R is singular or *flag != 0 (then -1).
struct CovPairTask {
  int role_a, idx_a, role_b, idx_b, slot, out;
};
// X may be null when there is no reduced system.
void launch_cov_pair_blocks(const DevProblem &P, const double *X, const double *scale, const double *Gb,
                            const double *Rb, const CovPairTask *tasks, int n_tasks, double *out, int *status,
                            const int *flag, hipStream_t s);

// ---- cov_lens.hip ----
// The same with the camera's l1, l2 estimated (DevCamL: the loaded problem's
// switch), the camera block three wide.
// After launch_cov_schur on the same stream: G_la = Q'L_a of every e-block into
// Glb (12 nc doubles; a = l1, l2 from cl.jrows_l) and the e-blocks' borders
// L_a'F_q - G_la'G_q into cl.cam_slab in k_schur_cam's layout;
// launch_schur_cam_gather then assembles reduced rows cam_row + 1, cam_row + 2
// (after launch_schur_gather; a diagonal of 0 on slots 1, 2 adds nothing there).
void launch_cov_schur_cam(const DevProblem &P, const DevCamL &cl, const double *scale, const double *Qb,
                          const double *Gb, double *Glb, hipStream_t s);
// launch_cov_blocks with the e-blocks' l columns (Glb) and cov_cam [9], the
// marginal of [f, l1, l2] (row-major, exactly symmetric), in place of var_f.
void launch_cov_blocks_lens(const DevProblem &P, const double *Z, const double *scale, const double *Gb,
                            const double *Rb, const double *Glb, double *cov_e, int *status_e, double *cov_f,
                            double *cov_cam, const int *flag, hipStream_t s);
// launch_cov_pair_rhs / launch_cov_pair_blocks with the camera (kCovFocal)
// three wide: three unit columns as a right-hand side, three rows as a, three
// columns as b, the rest 0.
void launch_cov_pair_rhs_lens(const DevProblem &P, const double *Gb, const double *Rb, const double *Glb,
                              const int2 *rhs, int n_rhs, double *B, hipStream_t s);
void launch_cov_pair_blocks_lens(const DevProblem &P, const double *X, const double *scale, const double *Gb,
                                 const double *Rb, const double *Glb, const CovPairTask *tasks, int n_tasks,
                                 double *out, int *status, const int *flag, hipStream_t s);

// ---- cov_direct.hip ----
// The mixed e-block set's direct groups (groups[0 .. n_groups), device; kind
// kMixDirect), after launch_cov_schur on the same stream: each group's plain
// F'F over [f | its tag blocks | its own pose | rhs = 0] into its slot of
// P.slab, whole.  scale: the own pose's comes from its f-block's slots.
void launch_cov_direct(const DevProblem &P, const double *scale, const int *groups, int n_groups, hipStream_t s);

}  // namespace arslam
