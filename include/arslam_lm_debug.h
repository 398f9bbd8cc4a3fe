/*
 * arslam_lm_debug.h -- component entry points of libarslam_lm.so used by the
 * parity tests to check one device stage at a time against the CPU oracle.
 * Not part of the drop-in boundary (arslam_lm.h); same error conventions.
 */
#ifndef ARSLAM_LM_DEBUG_H
#define ARSLAM_LM_DEBUG_H

#include "arslam_lm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Residuals and Jacobians of n independent observations on the device.
 * cam [n*3], cap [n*6], tag [n*6], corners [n*8] -> r [n*8],
 * J [n*8*15] row-major with columns cam(3) cap(6) tag(6), as ceres'
 * AutoDiffCostFunction<ArucoReprojectionError,8,3,6,6> would produce. */
int arslam_debug_residual_jacobian(int n, const double *cam, const double *cap, const double *tag,
                                   const double *corners, double *r, double *J);

/* The same rows for tags of side size[n] (metres, finite and > 0), through
 * the device functions the sized instances of k_linearize use.  At
 * ARSLAM_DEFAULT_TAG_SIZE r and J are arslam_debug_residual_jacobian's bits. */
int arslam_debug_residual_jacobian_sized(int n, const double *cam, const double *cap, const double *tag,
                                         const double *corners, const double *size, double *r, double *J);

/* The same rows under a camera model (arslam_lm.h ARSLAM_CAMERA_*; cam [n*3]
 * = f, l1, l2 per observation), through the device functions the kDist
 * instances of k_linearize use; size [n] as above, or NULL for the default
 * side.  Columns 1 and 2 of J (l1, l2) are 0 under either model.  Under
 * ARSLAM_CAMERA_PINHOLE r and J are arslam_debug_residual_jacobian's (or
 * _sized's) bits. */
int arslam_debug_residual_jacobian_model(int n, int model, const double *cam, const double *cap, const double *tag,
                                         const double *corners, const double *size, double *r, double *J);

/* The two distortion columns of the radial model's rows, which
 * arslam_debug_residual_jacobian_model leaves zero (they are held there):
 * Jl[(8 i + row) * 2 + a] = d r / d l1 (a = 0), d r / d l2 (a = 1) for
 * observation i; r as arslam_debug_residual_jacobian_model(RADIAL) returns it.
 * size: null = every tag of ARSLAM_DEFAULT_TAG_SIZE. */
int arslam_debug_residual_jacobian_distortion(int n, const double *cam, const double *cap, const double *tag,
                                              const double *corners, const double *size, double *r, double *Jl);

/* The same rows after each observation's robust loss (arslam_lm.h
 * ARSLAM_LOSS_*; kind [n], a [n]), through the device functions k_linearize
 * uses: r [n*8] and J [n*8*15] times sqrt(rho'(s)), s = |r|^2 over the
 * observation's 8 residuals, and rho [n] = rho(s) (the observation's cost is
 * rho / 2). */
int arslam_debug_residual_jacobian_loss(int n, const double *cam, const double *cap, const double *tag,
                                        const double *corners, const unsigned char *kind, const double *a,
                                        double *r, double *J, double *rho);

/* ceres::AngleAxisRotatePoint (rotation.h; called at ar_slam_util.cpp:145,155)
 * of n points p[n*3] by angle-axis w[n*3] on the device -> out[n*3], and the
 * branch each took: branch[i] = 1 if theta^2 > DBL_EPSILON (Rodrigues), 0 for
 * the first-order form x + w x p. */
int arslam_debug_angle_axis_rotate(int n, const double *w, const double *p, double *out, int *branch);

/* Dense reduced-system solve on the device: factor the lower triangle of the
 * n x n row-major SPD matrix A (in place: on return A holds L) and solve
 * A y = b.  *info = 0 on success, k+1 if pivot k was not positive. */
int arslam_debug_dense_llt(long n, double *A, const double *b, double *y, int *info);
/* the same with the factorization executor chosen (0 level launches, 1 persistent task graph);
 * info < 0 reports a task-graph wait that timed out */
int arslam_debug_dense_llt_ex(long n, double *A, const double *b, double *y, int *info, int executor);

/* Facts of a tile plan, as the two entries below built it. */
typedef struct {
  int tiles_per_side;
  long n_assembled;   /* tiles of the taken pattern (a two-phase plan: of the class-1 columns) */
  long n_tiles;       /* tiles of the factor, after symbolic fill */
  int n_levels;       /* level launches (a two-phase plan: both phases' lists) */
  long n_split;       /* update targets whose k-list is split into chunks */
  long n_dag_tasks;   /* tasks of the persistent executor's graph */
  int fill_first_ok;  /* 1: every fill tile's first application is an unfolded update item */
  long phase_split;   /* tickets [0, phase_split) are phase 0 (one phase: = n_dag_tasks) */
  int grid[2];        /* workgroups of the k_factor_dag launch, or of the phase 0 / phase 1 launches;
                         0 where nothing is launched (level executor, an empty phase).  tile_plan:
                         for a request of 512, not clamped by a device */
  long n_cont_tasks;  /* tasks whose workgroup may go straight on to a continuation target */
  int dag_valid;      /* tile_plan only: as arslam_plan_info.dag_valid */
} arslam_tile_plan_facts;

/* The general form of arslam_debug_dense_llt_ex (which calls it with no pattern, classes or
 * flags): factor the n x n row-major SPD matrix A on a tile pattern as the reduced system is
 * factored (64 x 64 tiles, b as row n with pivot 1e300, identity padding after it) and solve
 * A y = b.
 * tile_pattern: NULL (dense) or T*T bytes, T = (n + 1 + 63) / 64, non-zero where lower tile
 *   (i, j), j <= i, of A is taken; A is not read elsewhere, nor above its diagonal.  Diagonal
 *   tiles and the whole last tile row (it holds row n) are always taken.
 * executor: 0 level launches, 1 persistent task graph and persistent backward solve.
 * col_class: NULL, or T bytes, 0 own subtree / 1 replicated top: the two-phase plan of a
 *   multi-rank solve on one rank -- phase 0, then phase 1 with no exchange between them.
 *   Executor 1 only; the class-1 columns must be closed under the elimination tree's parent.
 * flags bit 0: the fill-first store, as the solver runs it -- first_store = n_assembled, and
 *   the fill tiles are uploaded as quiet NaNs instead of zeros, so a read of a fill tile before
 *   its first store poisons the factor.  Executor 1, one phase, and a plan with fill_first_ok.
 * A broken rule above is ARSLAM_E_INVALID_ARG.
 * L_out [n*n]: the factor on its tiles, 0 elsewhere (may be A itself).  y [n].  pattern_out
 * (nullable) [T*T]: the pattern after fill.  *info: 0, k + 1 if pivot k was not positive, < 0 a
 * task-graph wait that timed out.  facts: nullable. */
int arslam_debug_tile_llt(long n, const double *A, const double *b, const unsigned char *tile_pattern,
                          int executor, const unsigned char *col_class, unsigned flags, double *L_out,
                          double *y, unsigned char *pattern_out, int *info, arslam_tile_plan_facts *facts);
/* Host only (no HIP call): the plan arslam_debug_tile_llt would build for T tiles a side, its
 * pattern after fill (pattern_out, nullable) and its facts, with dag_valid from the ticket-order
 * check and the simulated interleavings. */
int arslam_debug_tile_plan(int T, const unsigned char *tile_pattern, const unsigned char *col_class,
                           unsigned char *pattern_out, arslam_tile_plan_facts *facts);

/* The selected inverse behind arslam_lm_covariance, alone: factor the n x n
 * row-major SPD matrix A as the reduced system is factored (64 x 64 tiles, a
 * zero right-hand side as row n, identity padding after it; level launches)
 * and compute Z = A^{-1} on the tiles of the factor (Takahashi recursion).
 * tile_pattern: NULL for a dense matrix, else T*T bytes, T = (n + 1 + 63) / 64,
 * non-zero where lower tile (i, j), j <= i, of A is taken (A's entries
 * elsewhere are not read; diagonal tiles are always taken).  Z_out [n*n]: both
 * triangles of Z on the factor's tiles, 0 on the others.  pattern_out (may be
 * NULL) [T*T]: the factor's lower tile pattern, the given one after symbolic
 * fill.  *info = 0 on success, k+1 if pivot k was not positive. */
int arslam_debug_selinv(long n, const double *A, const unsigned char *tile_pattern, double *Z_out,
                        unsigned char *pattern_out, int *info);

/* The multi-right-hand-side tile solve behind arslam_lm_covariance_pairs,
 * alone: factor A exactly as arslam_debug_selinv does (zero right-hand side
 * as row n, identity padding, optional tile pattern with symbolic fill) and
 * return X = A^{-1} B from the forward and backward solve kernels over the
 * factor's tiles.  B, X_out [n*nrhs] row-major; the columns travel sixty to a
 * 64-column panel, as the covariance's blocks do.  info as in
 * arslam_debug_selinv. */
int arslam_debug_tile_solve(long n, const double *A, const unsigned char *tile_pattern, int nrhs, const double *B,
                            double *X_out, int *info);

/* The loaded problem's reduced rows, by the caller's blocks (one rank; any
 * elimination, a mixed set included): cap_row [n_cap], tag_row [n_tag] = the
 * first of the block's 6 rows in the reduced system, -1 for a block that is
 * eliminated, constant or unused (eliminated: free and -1); *cam_row = the focal's row (l1, l2 follow it), -1 if
 * the camera is not free.  Each nullable.  The order in which a reference has
 * to eliminate to reproduce arslam_lm_cov_info.min_pivot. */
int arslam_lm_debug_reduced_rows(arslam_lm *h, int *cap_row, int *tag_row, int *cam_row);

/* The camera's three rows of the assembled reduced system of the loaded
 * problem (one rank, a free camera) at its loaded point, under the Jacobi
 * scale of that point and the given trust-region radius: the linearization,
 * the Schur elimination and the gathers (with arslam_lm_set_estimate_distortion
 * in effect also the l1, l2 border), and nothing more -- no factorization.
 * n_cols must be the reduced row count + 1 (camera row + 4).
 * rows[b * n_cols + col], b = 0 (f), 1 (l1), 2 (l2): the symmetric matrix's
 * entry against reduced column col < n_cols - 1 (the LM diagonal included),
 * and at col = n_cols - 1 the row's right-hand side entry.  row_slot[3]: the
 * rows' parameter slots (0, 1, 2).  Without the switch rows 1, 2 hold their
 * D^2 alone.  The next solve starts from the loaded state as usual. */
int arslam_lm_debug_camera_rows(arslam_lm *h, double radius, long n_cols, double *rows, int *row_slot);

/* The same three rows of the covariance's reduced system: after a completed
 * solve (the preconditions of arslam_lm_covariance_lens), at the point it
 * returned, under that solve's Jacobi scale and with no LM diagonal -- the
 * covariance's linearization, its orthogonal elimination, with l1, l2 live
 * its border (k_cov_schur_cam), and the gathers, and nothing more: no
 * factorization.  rows, n_cols and row_slot as arslam_lm_debug_camera_rows;
 * the right-hand side entries are 0.  With l1, l2 held rows 1, 2 hold the
 * pivot 1 alone.  ARSLAM_E_STATE for a problem without a gauge anchor.  The
 * next solve starts from the loaded state as usual. */
int arslam_lm_debug_cov_camera_rows(arslam_lm *h, long n_cols, double *rows, int *row_slot);

/* Every stage of one LM step of the loaded problem (one rank; SoA or
 * pointer-keyed; any elimination; with or without a free camera or a reduced
 * system) at its loaded point under the given radius, as solve()'s first step
 * launches them: the linearization, the Jacobi scale with the LM diagonal, the
 * Schur elimination and its gathers in prep mode over a system cleared in
 * every tile, the l1, l2 border where it is estimated, the factorization, the
 * backward solve, the back-substitution with the fused candidate cost, and the
 * reduction of the step's scalars.  Every array is nullable.
 * g, colnorm, scale, diag, xc [info.n]: by parameter slot in the caller's order
 *   (camera 3, captures 6 each, tags 6 each), whichever side is eliminated;
 *   xc is the candidate x + step.
 * S [info.n_padded^2]: the assembled system before the factorization, row
 *   major, both triangles, every row of the padded system (row n_reduced: the
 *   right-hand side and its pivot; the padding rows), 0 where the factor has
 *   no tile.  row_slot [info.n_reduced]: the caller's slot of a reduced row,
 *   -1 for an alignment padding row.  y [info.n_reduced]: the reduced solution.
 * Sizes first: call with every array null.  The next solve starts from the
 * loaded state and gives the bits it gives without this call. */
typedef struct {
  long n;                 /* the caller's parameter slots, 3 + 6 n_cap + 6 n_tag */
  int n_cap, n_tag;       /* the caller's blocks */
  long n_reduced;         /* rows of the reduced system, alignment padding included; 0: none */
  long n_padded;          /* tiles per side * 64 (> n_reduced); 0: none */
  int cam_row;            /* -1: the camera is not free */
  int elimination_used;   /* ARSLAM_ELIM_CAPTURES, _TAGS or _MIXED */
  int n_groups;           /* eliminated blocks + direct groups (the e-side of the device problem) */
  int n_direct;           /* direct groups of a mixed set */
  int n_big_groups;       /* groups on the second Schur launch (more than 10 distinct f-blocks) */
  int n_chunk_groups;     /* groups of more than 8 observations (the chunked instances) */
  int n_split_dest;       /* gather destinations summed in pieces */
  int max_contrib;        /* most contributions of one gather destination */
  long n_tiles, n_assembled_tiles;   /* tiles of the factor; of them assembled at the load */
  double cost, fixed_cost;           /* the linearization's */
  double model_cost_change, candidate_cost, candidate_fixed_cost, e_step2, f_step2;
  int e_step_bad, candidate_bad, f_step_bad, indefinite;   /* the step's flags */
} arslam_lm_step_info;
int arslam_lm_debug_step_stages(arslam_lm *h, double radius, arslam_lm_step_info *info, double *g, double *colnorm,
                                double *scale, double *diag, double *S, int *row_slot, double *y, double *xc);

/* The same on a sharded handle (several ranks, or arslam_lm_debug_force_multirank):
 * a COLLECTIVE call -- every rank calls it with the same radius and lin_exchange,
 * and it performs the step's collectives.  From the loaded point it runs the
 * launches of solve()'s iteration 0 and first step on that path: the
 * linearization of the rank's own captures with its packed exchange, the Jacobi
 * scale with the LM diagonal, the Schur elimination assembling this rank's share,
 * D^2 on its own-subtree rows, phase 0 of the factorization, the all-reduce of
 * the top tiles, D^2 on the top rows, phase 1, the backward solve with its mask,
 * the back-substitution, and the all-gathered step scalars.
 * lin_exchange: 0 = iteration 0's sums are complete before the step (the packed
 *   all-reduce, used when no step follows a linearization); 1 = besides, a
 *   linearization of the same point is enqueued again as after an accepted step
 *   and its top-tag sums and camera partials ride in front of the top tiles, its
 *   cost and norms with the step's scalars (what a step that follows a
 *   linearization does).  g, colnorm and diag are then that linearization's.
 * info: as above, by the whole problem's blocks; n_groups, n_big_groups,
 *   n_chunk_groups, n_split_dest, max_contrib, n_tiles, n_assembled_tiles are this
 *   rank's; the scalars and flags are the exchanged ones (every rank's the same).
 * shard: {rank, n_ranks, n_top_tiles, n_top_rows (real rows of the replicated
 *   top), n_owned_captures, n_active_ranks, lin_exchange, 0}.
 * g, colnorm, scale, diag, xc [info.n]: by the whole problem's slots, 0 for the
 *   captures of other ranks.  held [info.n]: 1 where a slot's values mean
 *   something on this rank -- the captures it owns; the camera and tag slots whose
 *   reduced row lies in its own subtrees or in the replicated top (the top and,
 *   with it, the camera are held by EVERY rank); slots without a reduced row
 *   (constant or unseen blocks: the loaded bits on every rank).  A tag of another
 *   rank's subtree is not held: its sums are partial and its xc may be stale.
 * S [info.n_padded^2]: this rank's SHARE of the system, copied after D^2 went on
 *   its own-subtree rows and before phase 0.  Rows of class 0 (own subtrees) are
 *   final: their D^2, alignment padding rows as identity rows.  Top tiles (class
 *   1) hold the sum over this rank's captures alone: no D^2, and the rows the top
 *   carries besides -- padding, the right-hand side's pivot, the rows past it --
 *   have 0 on the diagonal (their pivots go on after the exchange).  The
 *   right-hand side row holds this rank's captures' part.  Rows of class 2
 *   (another rank's subtrees) have no tile here: 0.
 * row_slot, row_class [info.n_reduced]: the whole problem's slot of a row (-1:
 *   padding) and its class 0 / 1 / 2.  y [info.n_reduced]: the reduced solution
 *   after the mask -- the top rows and this rank's own rows, 0 elsewhere.
 * Sizes first: call with every array null (a collective call like any other).
 * The next solve on every rank gives the bits of a fresh handle's. */
int arslam_lm_debug_step_stages_sharded(arslam_lm *h, double radius, int lin_exchange, arslam_lm_step_info *info,
                                        int shard[8], double *g, double *colnorm, double *scale, double *diag,
                                        unsigned char *held, double *S, int *row_slot, int *row_class, double *y,
                                        double *xc);

/* The device times of the handle's last arslam_lm_evaluate / _evaluate_blocks
 * under options.phase_timing = 1 (HIP events on its stream), ms: the parameter
 * upload, k_eval_obs, k_eval_blocks, k_eval_tree (both launches), the copy
 * back.  ARSLAM_E_STATE when there was no such call (tools/evaluate_cost.py). */
int arslam_lm_debug_evaluate_times(arslam_lm *h, double ms[5]);

/* Host-only symbolic analysis of the reduced system (no device needed): the
 * row layout arslam_lm_load_soa would choose for problem p under the given
 * ordering (0 natural, 1 RCM, 2 nested dissection) and tile pattern
 * (skip_zero_tiles), its tile Cholesky plan, and optionally the first row of
 * each tag (tag_row[n_tag], -1 if the tag is not a parameter). */
typedef struct {
  long n_reduced;          /* rows of the reduced system (6 per free tag + 3 camera) */
  long n_padded;           /* tiles_per_side * 64 */
  long pad_rows;           /* alignment padding rows among the tag rows */
  int tiles_per_side;
  int n_parts;             /* ordering parts (ND leaves + separators) */
  int camera_row;          /* -1 if the camera is constant */
  int n_levels;            /* height of the tile elimination tree */
  long n_assembled_tiles;  /* tiles the Schur assembly writes */
  long n_factor_tiles;     /* after symbolic fill */
  long n_update_tiles;     /* (target, column) tile products per factorization */
  long n_update_items;     /* update work items (after splitting long k-lists) */
  long n_split_targets;
  double update_flops;     /* algorithmic flops of the trailing updates per factorization */
  long n_dag_tasks;        /* tasks of the persistent executor's graph */
  int dag_valid;           /* 1: run one at a time in ticket order, every wait is already met, and
                              every simulated interleaving finishes (grids 1..512 and the small-graph
                              grid, random and adversarial policies); -(grid * 16 + policy) of the
                              first simulated deadlock */
  double factor_flops;     /* flops of the tile plan per factorization (POTRF, TRSM, updates, inverses) */
  double scalar_flops;     /* flops of the scalar Cholesky of the real rows in this order (no padding,
                              no structurally zero entries inside tiles) */
  int fill_first_ok;       /* 1: every fill tile's first application is an unfolded update item, so the
                              solver leaves fill tiles uncleared and that update stores 0 - acc */
} arslam_plan_info;

/* diagnostic builds only (-DARSLAM_SCHUR_STAMPS): per-phase cycles of the
 * Schur kernel accumulated over all its waves (zeros otherwise) */
int arslam_debug_schur_stamps(unsigned long long out[16]);

/* Test hooks on a solver handle.
 * force_indefinite: at every linear solve i (0-based) whose bit
 * min(i, 63) is set in step_mask, the reduced system's first camera row
 * (the last row if the camera is constant) gets diagonal -1 after the LM
 * diagonal is added, so the Cholesky reports a failed pivot and the LM step
 * is invalid (Ceres' LinearSolver FAILURE path).  0 turns it off.
 * break_dependency: on a problem loaded by arslam_lm_load_soa with the
 * persistent executor, raise the first wait of the first task at or after
 * `ticket` that has one beyond any count it can reach; the next solve must
 * then fail with ARSLAM_E_DEVICE.  *broken = the task changed.  Load again
 * to repair. */
int arslam_lm_debug_force_indefinite(arslam_lm *h, unsigned long long step_mask);
int arslam_lm_debug_break_dependency(arslam_lm *h, long ticket, long *broken);
/* force_multirank: on = 1 makes the handle take the multi-rank path with one
 * rank -- the subtree split (the two-rank split's replicated top, everything
 * below it this rank's), the two-phase factorization and every collective of
 * a multi-rank solve -- so that arslam_lm_set_comm(h, 0, 1, id) creates a
 * one-rank RCCL communicator and the solver issues its real ncclAllReduce
 * calls (f64 SUM / MAX, u8 MAX) on its stream on a one-GPU box.  Resets the
 * communicator (set it again after this call); 0 restores the one-rank path. */
int arslam_lm_debug_force_multirank(arslam_lm *h, int on);
/* tag_pair_tile: on a pointer-keyed problem loaded with capture elimination
 * on one rank, where the coupling of tag blocks a and b (and the pair's
 * mirror) falls in the reduced system: *status = 2 a tile assembled at the
 * load, 1 a fill tile of the loaded factor (an appended capture coupling them
 * keeps the plan: the gather writes into the fill tile), 0 no tile of the
 * factor (an append reloads), -1 a or b is not a free tag of the loaded
 * problem. */
int arslam_lm_debug_tag_pair_tile(arslam_lm *h, const double *tag_a, const double *tag_b, int *status);

/* Ceres 2.0's DENSE_SCHUR e-block set for problem p (ComputeStableSchurOrdering,
 * the rule ARSLAM_ELIM_AUTO follows), host only: out = {captures, tags,
 * camera (0/1) in the set, most observations of one tag}. */
int arslam_debug_ceres_e_blocks(const arslam_soa_problem *p, int out[4]);

/* Host only: the set itself (e_cap[n_cap], e_tag[n_tag]: 1 = eliminated) and the
 * ARSLAM_ELIM_MIXED device problem built from it: out = {groups (eliminated
 * captures + eliminated tags + direct groups), reduced-side blocks, direct
 * groups, most local blocks of one group}. */
int arslam_debug_mixed_groups(const arslam_soa_problem *p, int out[4], unsigned char *e_cap, unsigned char *e_tag);

int arslam_debug_reduced_plan(const arslam_soa_problem *p, int ordering, int skip_zero_tiles,
                              arslam_plan_info *info, int *tag_row);
/* Host only: the reduced layout (nested dissection, sparse tiles) and tile plan
 * of p's device problem under elimination (ARSLAM_ELIM_CAPTURES, _TAGS or
 * _MIXED: Ceres' set), built as a fresh one-rank load builds it.  Returns the
 * side used (MIXED falls back to a whole side as the load does) or an error. */
int arslam_debug_reduced_plan_side(const arslam_soa_problem *p, int elimination, arslam_plan_info *info);

/* Host only: the elimination-order memory of a handle over a sequence of
 * loads.  problems[0] is laid out as a first one-rank load lays it out under
 * elimination (as above) and ordering (sparse tiles); each later one as a
 * pointer-keyed reload of a grown problem, which may keep the remembered
 * order.  forget_before (nullable) [n_problems]: non-zero drops the memory
 * before that load, as arslam_lm_reset does.  Per problem: steps[i], and the
 * first reduced row of each of the caller's blocks, -1 where the block has
 * none: tag_row[i] [n_tag], cap_row[i] [n_cap] (captures have rows under tag
 * elimination and in a mixed set); the arrays and their entries are nullable. */
typedef struct {
  int side;           /* the side used (MIXED falls back to a whole side as the load does) */
  int order_reused;   /* as arslam_lm_summary.order_reused */
  int recomputed;     /* 1: a kept order made the tile elimination tree too tall and was replaced */
  int etree_height;   /* levels of the tile elimination tree */
  long pad_rows;      /* as arslam_plan_info.pad_rows */
} arslam_order_step;
int arslam_debug_order_memory(const arslam_soa_problem *problems, int n_problems, int elimination, int ordering,
                              const unsigned char *forget_before, arslam_order_step *steps, int *const *tag_row,
                              int *const *cap_row);

/* Host only: one simulated interleaving of n_workers workgroups running the
 * persistent executor's protocol on the one-rank plan of p (policy 0 random,
 * 1-3 adversarial orders; + 16 drops the cap on claimed continuations in
 * flight, which the protocol relies on).  *ok = 1 if every task finished, 0 on
 * a deadlock. */
int arslam_debug_dag_simulate(const arslam_soa_problem *p, int n_workers, unsigned seed, int policy, int *ok);
/* The same with only n_started of the grid's n_workers workgroups ever
 * starting (each when the schedule picks it): fewer workgroups resident than
 * the grid.  The executor caps claimed continuations at half the workgroups
 * started so far; policy + 32 simulates round 5's cap (half the grid), which
 * such schedules deadlock. */
int arslam_debug_dag_simulate_started(const arslam_soa_problem *p, int n_workers, int n_started, unsigned seed,
                                      int policy, int *ok);
/* Process-wide: every later k_factor_dag launch lets only its first k
 * workgroups start (the others return at once), as if only k were resident;
 * k <= 0 restores the whole grid.  The factorization's result does not depend
 * on it (fixed summation order). */
int arslam_debug_dag_workgroup_limit(int k);

/* Host only: the message an executor fault carries for the one-rank plan of p
 * (nested dissection, sparse tiles) and a fault record rec[9] = {ticket, kind
 * (1 dependency wait, 2 in-order application, 3 late wait), counter, value
 * seen, value awaited, tickets drawn, claimed continuations in flight,
 * workgroup, INT_MAX - the smallest ticket whose wait ran out of time (0:
 * none)}: the task, the counter, the tickets that advance it.  Writes at most
 * len bytes (NUL-terminated) to buf. */
int arslam_debug_dag_fault_detail(const arslam_soa_problem *p, const int rec[9], char *buf, int len);

/* The memory round trips of the persistent executor's hand-offs on this
 * device, measured in a few milliseconds (one lane each): out = {never-matching
 * CAS poll (ns, dependent chain), agent-scope sc1 load (ns, dependent chain),
 * write-through store + its acknowledgement (ns each), workgroup ping-pong
 * through agent-scope flags (ns per round trip, -1 if it timed out), the two
 * workgroups' XCC ids}.  device < 0: the current device. */
int arslam_debug_box_fingerprint(int device, double out[6]);

/* Host only: the multi-rank split arslam_lm_load_soa makes for rank `rank` of
 * `nranks` (nested dissection, sparse tiles) -- its two-phase tile plan, and
 * every capture's owning rank (cap_owner[n_cap], may be NULL). */
typedef struct {
  int tiles_per_side;
  int n_top_cols;           /* tile columns replicated on every rank */
  int n_own_cols;           /* tile columns of this rank's subtrees */
  long n_top_tiles;         /* tiles of the top columns (the per-step exchange) */
  long n_tiles;             /* tiles stored on this rank (top + own) */
  long n_dag_tasks, phase_split;   /* tasks of the plan; [0, phase_split) run before the exchange */
  int dag_valid;            /* 1: ticket order valid and the randomised interleavings finish */
  int n_owned_captures;
  double top_work, max_rank_work, total_work;   /* tile-task counts (RankSplit) */
  int n_active;             /* ranks owning subtrees (the others own top-only captures) */
} arslam_split_info;
int arslam_debug_rank_split(const arslam_soa_problem *p, int nranks, int rank, arslam_split_info *info,
                            int *cap_owner);
/* Host-only: the factorization's task graph in the plan the solver makes for
 * `rank` of `nranks` (1: the one-rank plan), in ticket order: tasks[4 t ..] =
 * {type, y, z, w} (0 POTRF k = y; 1 TRSM; 2 update item; 3 INV k = y) and
 * phase[t], for the first `cap` tickets; *n_tasks the plan's count; info =
 * {tile columns T, phase_split, phases, the column whose POTRF task also
 * inverts L_kk and that has no INV task (-1: none)}. */
int arslam_debug_dag_tasks(const arslam_soa_problem *p, int nranks, int rank, int *tasks, int *phase, long cap,
                           long *n_tasks, int info[4]);
/* Host-only: the Schur gather plan of p's first c0 captures (their residual
 * blocks, p's order), extended by captures c0.. (schur_gather_extend, the
 * appended-problem path), against the plan built afresh for all of p with the
 * same layout.  *identical = 1 when every array agrees; *n_dest the
 * destinations of the full plan. */
int arslam_debug_gather_extend(const arslam_soa_problem *p, int c0, int *identical, int *n_dest);
/* Host only: the descriptors of the Schur kernel's output stage for a capture
 * of nblk distinct tags (1..10), as the kernel reads them: 13 tiles (r, cc),
 * cc <= r + 1, of its 16x16 output product in that order, 64 lanes, 4
 * registers -- lane (lk, li) holds element (16 r + lk + 4 reg, 16 cc + li) of
 * the capture's local system.  off[13*64*4]: the element's offset in the
 * capture's block-packed slab; stored[13*64*4]: 1 where the lane stores it
 * (the lower block triangle), 0 elsewhere (off is then meaningless). */
int arslam_debug_schur_store_table(int nblk, int *off, unsigned char *stored);

#ifdef __cplusplus
}
#endif
#endif
