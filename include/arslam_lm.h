/*
 * arslam_lm.h -- C-ABI of the MI355X-native Levenberg-Marquardt bundle
 * adjuster that replaces ar_slam's ceres::Solve call.
 *
 * Drop-in boundary.  The reference builds a ceres::Problem
 * and hands it to ceres::Solve:
 *
 *   AddResidualBlock(AutoDiff<ArucoReprojectionError,8,3,6,6>, nullptr,
 *                    camera, capture.inv_pose, aruco.pose)
 *        ar_slam_util.cpp:720-727, 829-836, 956-963
 *   SetParameterBlockConstant(block)       ar_slam_util.cpp:965, 972
 *   ceres::Solve(options, &problem_, &s)   ar_slam_util.cpp:1001-1018
 *   resetProblem()                         ar_slam_util.cpp:1021-1025
 *
 * Each entry point below replaces one of those calls with the same argument
 * meaning: parameter blocks are caller-owned double arrays keyed by their
 * address (camera[3] = f,l1,l2 -- f is estimated; l1 and l2 are used under
 * ARSLAM_CAMERA_RADIAL only, held constant there unless
 * arslam_lm_set_estimate_distortion is on; capture[6] = inv_pose
 * t,w; tag[6] = pose t,w), observations are copied (as the functor copies its ArucoRect,
 * ar_slam_util.cpp:194-196), and results are written back into the caller's
 * arrays when the solve ends (Ceres' default; update_state_every_iteration
 * writes them after every improving step).
 *
 * Conventions: every function returns 0 (ARSLAM_OK) or a negative
 * ARSLAM_E_* code; no C++ exception crosses the ABI; a handle is not
 * thread-safe.  arslam_lm_last_error() returns the message of the most
 * recent failure on the calling thread.
 */
#ifndef ARSLAM_LM_H
#define ARSLAM_LM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARSLAM_LM_MAX_ITERS 1024
#define ARSLAM_COMM_ID_BYTES 128

enum {
  ARSLAM_OK = 0,
  ARSLAM_E_INVALID_ARG = -1,
  ARSLAM_E_UNSUPPORTED = -2,
  ARSLAM_E_NO_DEVICE = -3,
  ARSLAM_E_HIP = -4,
  ARSLAM_E_OUT_OF_MEMORY = -5,
  ARSLAM_E_COMM = -6,
  ARSLAM_E_STATE = -7,
  ARSLAM_E_DEVICE = -8          /* a device executor fault (a dependency wait that never completed) */
};

/* Which side of the capture/tag graph the Schur complement eliminates
 * (DENSE_SCHUR's e-blocks, ar_slam_util.cpp:1011).  AUTO follows Ceres 2.0's
 * own choice (ReorderProgramForSchurTypeLinearSolver -> ComputeStableSchurOrdering:
 * the stable greedy independent set of the Hessian graph in ascending degree,
 * blocks in program order): the side that holds the majority of that set is
 * eliminated (Ceres may mix the two sides; the step is the same exact solve of
 * the same system, only the rounding differs).  MIXED eliminates exactly
 * Ceres' set -- captures and tags together when it mixes them (residuals
 * joining two reduced-side blocks then go straight into the reduced system, as
 * in Ceres' SchurEliminator); summary.elimination_used then reports MIXED, or
 * the side when the set is one whole side.  Multi-rank solves always
 * eliminate captures (the shards are capture ranges); MIXED is single-rank. */
enum { ARSLAM_ELIM_AUTO = 0, ARSLAM_ELIM_CAPTURES = 1, ARSLAM_ELIM_TAGS = 2, ARSLAM_ELIM_MIXED = 3 };

/* Ceres termination types (ceres::TerminationType) */
enum { ARSLAM_CONVERGENCE = 0, ARSLAM_NO_CONVERGENCE = 1, ARSLAM_FAILURE = 2, ARSLAM_USER_SUCCESS = 3,
       ARSLAM_USER_FAILURE = 4 };

/* summary.setup_kind: a full load (structure, elimination order, plan), the
 * loaded problem with new values only, or an appended problem whose new
 * residual blocks fit the loaded tile pattern (order and plan kept) */
enum { ARSLAM_SETUP_LOAD = 0, ARSLAM_SETUP_VALUES = 1, ARSLAM_SETUP_APPEND = 2 };

/* which termination test fired */
enum {
  ARSLAM_RULE_NONE = 0, ARSLAM_RULE_GRADIENT = 1, ARSLAM_RULE_PARAMETER = 2,
  ARSLAM_RULE_FUNCTION = 3, ARSLAM_RULE_MIN_RADIUS = 4, ARSLAM_RULE_MAX_ITERS = 5,
  ARSLAM_RULE_INVALID_STEPS = 6, ARSLAM_RULE_EVAL_FAILED = 7, ARSLAM_RULE_USER_CALLBACK = 8
};

/* ceres::LossFunction of a residual block (Ceres 2.0 loss_function.cc), with
 * s = |r|^2 over the block's 8 residuals, scale a and b = a^2; the cost is
 * 1/2 sum rho(s):
 *   NONE        rho = s                          (the nullptr of AddResidualBlock)
 *   HUBER       rho = s (s <= b), 2 a sqrt(s) - b   ceres::HuberLoss(a)
 *   SOFT_L_ONE  rho = 2 b (sqrt(1 + s/b) - 1)       ceres::SoftLOneLoss(a)
 *   CAUCHY      rho = b log(1 + s/b)                ceres::CauchyLoss(a)
 * As in Ceres (corrector.cc; all three have rho'' <= 0) the linearization
 * uses sqrt(rho') r and sqrt(rho') J per block and the cost rho itself: the
 * gradient, Jacobi scaling, Schur complement, model cost change and step
 * quality all work on the corrected rows.  Later kinds (Tolerant, Tukey,
 * Arctan, Scaled, Composed) would append to the enum; any other value is
 * ARSLAM_E_INVALID_ARG today, and so is a scale that is not finite or not
 * > 0 for every kind but NONE (which ignores it). */
enum { ARSLAM_LOSS_NONE = 0, ARSLAM_LOSS_HUBER = 1, ARSLAM_LOSS_SOFT_L_ONE = 2, ARSLAM_LOSS_CAUCHY = 3 };

/* The side length of a tag, in metres: the functor's other constant
 * (ArucoReprojectionError(rect) plus a size; the reference fixes it,
 * aruco_size, ar_slam_util.hpp:319).  Corner i of a tag of side s is
 * 0.5 s ARUCO_DIRECTIONS[i] in the tag's frame.  The tag sides are the only
 * thing that gives the map its metric scale: the residual is unchanged when
 * every translation and every side are scaled together.  A residual block
 * carries the side of its tag, bound when the block is added, like its loss;
 * any side that is not finite or not > 0 is ARSLAM_E_INVALID_ARG. */
#define ARSLAM_DEFAULT_TAG_SIZE 0.0635
/* a side the API accepts: finite and > 0 (false for NaN) */
#define ARSLAM_TAG_SIZE_VALID(s) ((s) > 0.0 && (s) <= 1.7976931348623157e308)

/* The camera model of a handle's residual blocks.  PINHOLE, the default, is
 * the reference's projectCorner as it stands: u = f x, v = f y with
 * x = p_x / p_z, y = p_y / p_z, and camera[1], camera[2] ignored.  RADIAL is
 * the TODO it carries (ar_slam_util.cpp:164-171), with l1 = camera[1] and
 * l2 = camera[2] as a known calibration:
 *   r2 = x^2 + y^2,  d = 1 + r2 (l1 + l2 r2),  (u, v) = f d (x, y).
 * l1 and l2 are held constant by the solve (in Ceres terms a
 * SubsetParameterization of the camera block on {1, 2}): their Jacobian
 * columns are zero and the values the caller passes come back unchanged; f is
 * still estimated unless the camera block is constant.  No guard is added for
 * a polynomial that folds back: the calibration must be monotone over the
 * field of view, d + 2 r2 d' > 0 with d' = l1 + 2 l2 r2, as every observed
 * point must have p_z > 0.  Any other value is ARSLAM_E_INVALID_ARG. */
enum { ARSLAM_CAMERA_PINHOLE = 0, ARSLAM_CAMERA_RADIAL = 1 };
#define ARSLAM_CAMERA_MODEL_VALID(m) ((m) == ARSLAM_CAMERA_PINHOLE || (m) == ARSLAM_CAMERA_RADIAL)

/* ceres::Solver::Options subset used by ArSlamSolver::optimize
 * (ar_slam_util.cpp:1003-1012); defaults from arslam_lm_options_init are
 * the reference's values (max_num_iterations = 50, DENSE_SCHUR) plus Ceres
 * 2.0 defaults for everything it leaves unset. */
typedef struct {
  int max_num_iterations;
  double function_tolerance;
  double gradient_tolerance;
  double parameter_tolerance;
  double initial_trust_region_radius;
  double max_trust_region_radius;
  double min_trust_region_radius;
  double min_relative_decrease;
  double min_lm_diagonal;
  double max_lm_diagonal;
  int max_num_consecutive_invalid_steps;
  int jacobi_scaling;
  int elimination;                   /* ARSLAM_ELIM_* */
  int minimizer_progress_to_stdout;  /* Ceres progress table */
  int update_state_every_iteration;  /* write improving iterates back */
  int device;                        /* HIP device ordinal, -1 = current */
  int cholesky_skip_zero_tiles;      /* 1: skip structurally-zero tiles of the reduced system */
  int reduced_ordering;              /* tags in the reduced system: 0 natural, 1 reverse
                                        Cuthill-McKee, 2 nested dissection (default) */
  int kernel_timing;                 /* 1: HIP events around every launch of the dominant kernel */
  int factor_executor;               /* reduced-system Cholesky: 0 two launches per elimination-tree
                                        level, 1 one persistent task-graph launch (default) */
  int phase_timing;                  /* 1: HIP events around each phase of the step (summary
                                        t_*_ms; host loop only); 0 (default): none (each event
                                        record costs a few microseconds of GPU time) */
} arslam_lm_options;

/* ceres::IterationSummary subset */
typedef struct {
  int iteration;
  double cost, cost_change, gradient_max_norm, gradient_norm, step_norm;
  double relative_decrease, trust_region_radius;
  int step_is_valid, step_is_successful;
  double iteration_time, cumulative_time;
} arslam_lm_iteration;

/* ceres::Solver::Summary subset plus per-phase device timings */
typedef struct {
  int termination;              /* ARSLAM_CONVERGENCE ... */
  int rule;                     /* ARSLAM_RULE_* */
  int num_successful_steps, num_unsuccessful_steps;
  int num_linear_solves;        /* trust-region step computations = LM iterations of the metric */
  double initial_cost, final_cost, fixed_cost;
  double final_rms_px;          /* sqrt(2 final_cost / (4 n_obs)); with a loss set final_cost is the
                                   robustified cost 1/2 sum rho(s), so this is the robustified figure */
  int n_obs, n_reduced;         /* residual blocks; size of the reduced (tag+camera) system */
  double setup_time_s;          /* host assembly + upload */
  int setup_kind;               /* ARSLAM_SETUP_*: how the problem reached the device for this solve */
  double minimizer_time_s;      /* first evaluation to termination */
  double total_time_s;
  /* accumulated device time per phase (ms), from HIP events */
  double t_linearize_ms, t_schur_ms, t_cholesky_ms, t_solve_ms, t_backsub_ms, t_cost_ms;
  /* dominant kernel (reduced-system trailing update on MFMA), kernel_timing = 1 only */
  double t_dominant_ms;         /* sum of its launch durations */
  double dominant_flops;        /* algorithmic flops of those launches */
  long n_dominant_launches;
  /* reduced-system tile plan (per factorization) */
  long n_factor_tiles;          /* 64x64 tiles of the factor that exist */
  int n_levels;                 /* levels of the tile elimination tree (launch pairs) */
  long n_update_tiles;          /* tile updates (MFMA work items) */
  double factor_update_flops;   /* useful flops of the trailing updates */
  double factor_scalar_flops;   /* flops of the scalar Cholesky of the real rows (the algorithmic count:
                                   no padding rows, no zeros inside fill tiles) per factorization */
  double comm_bytes;            /* multi-rank: bytes this rank all-reduced during the solve */
  int elimination_used;         /* ARSLAM_ELIM_CAPTURES, _TAGS or _MIXED (Ceres' set, both kinds) */
  int ceres_e_captures;         /* Ceres 2.0's e-block set for this problem (ComputeStableSchurOrdering): */
  int ceres_e_tags;             /*   captures and tags in it (the camera joins it only in degenerate graphs) */
  /* several ranks (subtree-to-rank split of the reduced system's elimination tree) */
  int n_ranks;
  int n_owned_captures;         /* captures this rank owns (every capture on one rank) */
  long n_top_tiles;             /* tiles of the replicated top columns: the per-step exchange is these */
  double split_top_work;        /* tile tasks of the top columns (replicated on every rank) */
  double split_max_rank_work;   /* tile tasks of the busiest rank's subtrees */
  double split_total_work;      /* tile tasks of the whole factorization */
  double t_factor_own_ms;       /* device time of the factorization's phase 0 (own subtrees) and */
  double t_factor_top_ms;       /*   phase 1 (the top), summed over the solve (phase_timing = 1) */
  int n_iters;                  /* entries in iters[], iteration 0 included */
  arslam_lm_iteration iters[ARSLAM_LM_MAX_ITERS + 1];
  double setup_phase_s[5];      /* the last full load (ARSLAM_SETUP_LOAD): problem structure (Ceres'
                                   e-block rule + host problem), elimination order (reduced layout; several
                                   ranks: + the split), tile plan + task graph, Schur gather plan + upload,
                                   the rest (stream, co-visibility bookkeeping) */
  long comm_calls;              /* multi-rank: collectives this rank made during the solve */
  int n_active_ranks;           /* ranks that own subtrees of the split (the others own only captures that
                                   see top tags alone); 1 on one rank */
  int order_reused;             /* the last full load kept the earlier elimination order (an incremental
                                   reload: 1) or computed a fresh one (0) */
} arslam_lm_summary;

/* Whole problem in struct-of-arrays form (bulk / benchmark path). */
typedef struct {
  int n_cap, n_tag, n_obs;
  double *camera;                  /* [3], updated in place */
  double *cap;                     /* [n_cap*6], updated in place */
  double *tag;                     /* [n_tag*6], updated in place */
  const int *obs_cap;              /* [n_obs] */
  const int *obs_tag;              /* [n_obs] */
  const double *corners;           /* [n_obs*8] centred pixels x0,y0..x3,y3 */
  int camera_const;
  const unsigned char *cap_const;  /* [n_cap] or NULL */
  const unsigned char *tag_const;  /* [n_tag] or NULL */
} arslam_soa_problem;

typedef struct arslam_lm arslam_lm;

/* Fill *opt with the reference's solver options. */
int arslam_lm_options_init(arslam_lm_options *opt);

/* new ceres::Problem (ArSlamSolver::problem_, ar_slam_util.hpp:473) */
int arslam_lm_create(arslam_lm **out, const arslam_lm_options *opt);
void arslam_lm_destroy(arslam_lm *h);

/* Per-solve options (the Solver::Options ArSlamSolver::optimize builds on
 * every call, ar_slam_util.cpp:1003-1012).  Changing device, reduced_ordering
 * or cholesky_skip_zero_tiles drops a problem loaded by arslam_lm_load_soa
 * (load again); the pointer-keyed problem is unaffected. */
int arslam_lm_set_options(arslam_lm *h, const arslam_lm_options *opt);
int arslam_lm_get_options(const arslam_lm *h, arslam_lm_options *opt);

/* problem_.AddResidualBlock(new AutoDiffCostFunction<ArucoReprojectionError,
 * 8,3,6,6>(new ArucoReprojectionError(rect)), nullptr, camera, capture, tag)
 * -- ar_slam_util.cpp:720-727.  corners = ArucoRect x0,y0,..,x3,y3. */
int arslam_lm_add_residual_block(arslam_lm *h, const double corners[8], double *camera,
                                 double *capture, double *tag);

/* The handle's default loss: what arslam_lm_add_residual_block gives the
 * blocks added afterwards (Ceres binds a loss at AddResidualBlock; a caller
 * that passed `new ceres::HuberLoss(a)` there calls set_loss(ARSLAM_LOSS_HUBER,
 * a) once) and what arslam_lm_load_soa gives every observation.  It drops a
 * problem loaded by arslam_lm_load_soa (load again), as arslam_lm_set_comm
 * does; arslam_lm_reset keeps it.  A rejected call leaves the handle as it was. */
int arslam_lm_set_loss(arslam_lm *h, int kind, double a);
int arslam_lm_get_loss(const arslam_lm *h, int *kind, double *a);

/* arslam_lm_add_residual_block with this block's own loss
 * (AddResidualBlock(cost, new ceres::CauchyLoss(a), camera, capture, tag)). */
int arslam_lm_add_residual_block_loss(arslam_lm *h, const double corners[8], double *camera,
                                      double *capture, double *tag, int kind, double a);

/* The handle's default tag side, ARSLAM_DEFAULT_TAG_SIZE on creation: what
 * arslam_lm_add_residual_block and _loss give the blocks added afterwards and
 * what arslam_lm_load_soa and _loss give every tag.  Like arslam_lm_set_loss
 * it drops a problem loaded by arslam_lm_load_soa, arslam_lm_reset keeps it,
 * and a rejected call leaves the handle as it was. */
int arslam_lm_set_tag_size(arslam_lm *h, double size);
int arslam_lm_get_tag_size(const arslam_lm *h, double *size);

/* The handle's camera model (ARSLAM_CAMERA_*), PINHOLE on creation: a property
 * of the handle, like the default tag side.  Changing it drops a problem
 * loaded by arslam_lm_load_soa* and any cached covariance; the next load (or
 * the next arslam_lm_solve of the pointer-keyed blocks) uses it, on every
 * path: appends, the three eliminations, losses, sized tags, several ranks,
 * arslam_lm_covariance and arslam_lm_covariance_pairs.  arslam_lm_reset keeps
 * it.  An unknown value returns ARSLAM_E_INVALID_ARG and leaves the handle as
 * it was.  A PINHOLE problem launches the kernels it always launched.
 * (ARSLAM_E_UNSUPPORTED, handle unchanged: RADIAL on a handle of several ranks
 * whose arslam_lm_set_estimate_distortion is on.) */
int arslam_lm_set_camera_model(arslam_lm *h, int model);
int arslam_lm_camera_model(const arslam_lm *h, int *model);

/* "Estimate the distortion", off (0) on creation: a property of the handle,
 * like the camera model.  It takes effect only for a problem loaded under
 * ARSLAM_CAMERA_RADIAL; under PINHOLE the two columns are zero and the switch
 * is ignored.  With it on and the camera block not constant, l1 and l2 are
 * parameters like f (Ceres' AutoDiffCostFunction<..., 8, 3, 6, 6> with the
 * distortion in projectCorner): their columns d(u, v)/dl1 = f r^2 (x, y) and
 * d(u, v)/dl2 = f r^4 (x, y) enter the gradient, the Jacobi scale, the LM
 * diagonal, the reduced system, the step and its norms, and the caller's
 * camera[1], camera[2] come back estimated (start them at zero or at a
 * guess).  A constant camera block holds all three.  Off: the values passed
 * come back unchanged, by the kernels the handle always launched.
 * Changing it drops a problem loaded by arslam_lm_load_soa* and any kept
 * covariance; arslam_lm_reset keeps it.  A value other than 0 or 1 returns
 * ARSLAM_E_INVALID_ARG and leaves the handle as it was.
 * Limits while it is in effect, each ARSLAM_E_UNSUPPORTED with the handle
 * left as it was: several ranks (arslam_lm_set_comm, _set_comm_callback; the
 * switch itself on a handle that has them); ARSLAM_ELIM_MIXED on a problem
 * whose e-block set mixes captures and tags (a set that is one whole side is
 * solved); arslam_lm_covariance, _covariance_block, _covariance_pairs and
 * _covariance_block_pair, whose outputs have one scalar for the camera.  Their
 * _lens forms (below) carry the camera block whole and work under the switch.
 * An appended pointer-keyed problem is loaded in full (setup_kind says so). */
int arslam_lm_set_estimate_distortion(arslam_lm *h, int on);
int arslam_lm_estimate_distortion(const arslam_lm *h, int *on);

/* arslam_lm_add_residual_block_loss with this block's own tag side (every
 * block of one tag would pass the same; the side belongs to the block, as
 * to a Ceres functor). */
int arslam_lm_add_residual_block_sized(arslam_lm *h, const double corners[8], double *camera,
                                       double *capture, double *tag, double size, int kind, double a);

/* problem_.SetParameterBlockConstant(block) -- ar_slam_util.cpp:965, 972 */
int arslam_lm_set_parameter_block_constant(arslam_lm *h, double *block);
int arslam_lm_set_parameter_block_variable(arslam_lm *h, double *block);

/* ceres::Solve(options, &problem_, &summary) -- ar_slam_util.cpp:1015 */
int arslam_lm_solve(arslam_lm *h, arslam_lm_summary *summary);

/* ArSlamSolver::resetProblem -- ar_slam_util.cpp:1021-1025 */
int arslam_lm_reset(arslam_lm *h);

int arslam_lm_num_residual_blocks(const arslam_lm *h);

/* Bulk path: load an SoA problem into device memory once (HBM-resident), then
 * solve it any number of times from the loaded initial state; results are
 * written to the SoA arrays given at load time. */
int arslam_lm_load_soa(arslam_lm *h, const arslam_soa_problem *p);
int arslam_lm_solve_loaded(arslam_lm *h, arslam_lm_summary *summary);
/* arslam_lm_load_soa with one loss per observation, in p's observation order
 * (obs_loss_kind[n_obs] ARSLAM_LOSS_*, obs_loss_a[n_obs]); NULL for both: the
 * handle's default loss for every observation.  Several ranks: every rank
 * passes the whole problem's arrays, as it does the problem. */
int arslam_lm_load_soa_loss(arslam_lm *h, const arslam_soa_problem *p,
                            const unsigned char *obs_loss_kind, const double *obs_loss_a);

/* arslam_lm_load_soa_loss with one side per tag (tag_size[n_tag], metres);
 * NULL: the handle's default side for every tag.  A problem whose sides are
 * all ARSLAM_DEFAULT_TAG_SIZE runs the same kernels as one loaded without. */
int arslam_lm_load_soa_sized(arslam_lm *h, const arslam_soa_problem *p, const double *tag_size,
                             const unsigned char *obs_loss_kind, const double *obs_loss_a);

/* One-shot bulk solve (a handle of its own, so no loss: with one, create a
 * handle, arslam_lm_set_loss or arslam_lm_load_soa_loss, arslam_lm_solve_loaded). */
int arslam_lm_solve_soa(arslam_soa_problem *p, const arslam_lm_options *opt,
                        arslam_lm_summary *summary);

/* Multi-GPU (one process per GPU): every rank loads the WHOLE problem (the
 * same arslam_soa_problem / the same residual blocks) and the solver splits
 * it: the elimination tree of the reduced tag+camera system is cut below its
 * top separators, each rank owns some of the subtrees below the cut and the
 * captures whose tags lie in them, factors those columns, and the ranks then
 * sum only the top columns' tiles over RCCL before factoring the top
 * (replicated).  Results are written back for the rank's own captures
 * (arslam_lm_owned_captures) and for the camera and every tag. */
int arslam_comm_unique_id(unsigned char id[ARSLAM_COMM_ID_BYTES]);
int arslam_lm_set_comm(arslam_lm *h, int rank, int nranks,
                       const unsigned char id[ARSLAM_COMM_ID_BYTES]);

/* The same exchange through a caller-supplied host all-reduce (MPI, gloo,
 * ...): the solver stages each device buffer to host memory, calls
 * fn(ctx, buf, count, dtype, op) -- reduce `count` elements of `buf` in
 * place over all ranks, return 0 on success -- and copies the result back.
 * For ranks that share one GPU (RCCL needs one GPU per rank) and for tests.
 * Like arslam_lm_set_comm, this drops a loaded problem (load again).  Either
 * call with more than one rank is ARSLAM_E_UNSUPPORTED, the handle unchanged,
 * while arslam_lm_set_estimate_distortion is in effect. */
enum { ARSLAM_DT_F64 = 0, ARSLAM_DT_U8 = 1 };
enum { ARSLAM_OP_SUM = 0, ARSLAM_OP_MAX = 1 };
typedef int (*arslam_allreduce_fn)(void *ctx, void *buf, size_t count, int dtype, int op);
int arslam_lm_set_comm_callback(arslam_lm *h, int rank, int nranks, arslam_allreduce_fn fn, void *ctx);

/* The captures (indices into the loaded problem) this rank owns, ascending;
 * *n = their count (writes <= cap).  One rank owns every capture. */
int arslam_lm_owned_captures(const arslam_lm *h, int *out, int cap, int *n);

/* ceres::IterationCallback (Solver::Options::callbacks; the reference installs
 * one for its debug display, ar_slam_util.cpp:982-998, 1006-1009): called
 * after every iteration is recorded (iteration 0 included), before the
 * termination tests, with the parameter blocks already written back when
 * update_state_every_iteration is set.  Return ARSLAM_SOLVER_CONTINUE,
 * ARSLAM_SOLVER_ABORT (termination ARSLAM_USER_FAILURE) or
 * ARSLAM_SOLVER_TERMINATE_SUCCESSFULLY (ARSLAM_USER_SUCCESS).  fn = NULL
 * removes it.  Runs on the calling thread, inside arslam_lm_solve*. */
enum { ARSLAM_SOLVER_CONTINUE = 0, ARSLAM_SOLVER_ABORT = 1, ARSLAM_SOLVER_TERMINATE_SUCCESSFULLY = 2 };
typedef int (*arslam_iteration_callback)(void *ctx, const arslam_lm_iteration *it);
int arslam_lm_set_iteration_callback(arslam_lm *h, arslam_iteration_callback fn, void *ctx);

/* ---- marginal pose covariances (ceres::Covariance) ----
 * What ceres::Covariance::Compute after Solve, then GetCovarianceBlock(p, p)
 * for every pose block p and the camera, would give
 * (Covariance::Options::apply_loss_function = true).  At the parameters the
 * last solve returned, H = J~'J~ over every active residual block and every
 * free parameter -- the focal f if the camera is free and used (never l1, l2:
 * they are held constant, used under ARSLAM_CAMERA_RADIAL), 6 per free capture, 6 per free tag -- the
 * Jacobian rows corrected by sqrt(rho'(s)) exactly as the solve corrects them,
 * no LM diagonal.  C = H^-1, for unit-variance residuals: with pixel noise
 * sigma, multiply by sigma^2.  Only the marginals are returned: the 6x6
 * diagonal block of C of every free capture ([t_c, w_c], row-major) and tag
 * ([t_t, w_t]), and var(f).  C[i][j] and C[j][i] are the same bits.
 *
 * Gauge: the mapping problem has a 6-DoF gauge freedom unless a pose block is
 * held constant (arslam_lm_set_parameter_block_constant / cap_const /
 * tag_const).  As with Ceres' Cholesky-based covariance, a gauge-free problem
 * has no covariance; the result is the covariance in the anchor's gauge.  The
 * host checks this structurally before any device work (a union-find, no
 * threshold): every connected component of the capture-tag graph over the
 * active observations must contain a constant pose block, else the status is
 * ARSLAM_COV_RANK_DEFICIENT.  Behind it a numeric test: the factorization of
 * the reduced system (Jacobi-scaled, no LM diagonal) must raise no
 * non-positive pivot, and the smallest squared pivot of its real rows
 * (min_pivot; the rows of l1 / l2, the padding and the right-hand side
 * excluded) must be >= 1e-14.  This threshold stands where Ceres tests
 * singular values against min_reciprocal_condition_number = 1e-14; it is NOT
 * the same number (a pivot of the scaled Cholesky, not a ratio of singular
 * values).
 *
 * The device work: one linearization at the returned point, the reduced
 * system (each eliminated block by an orthogonal factorization of its
 * columns, not the LM step's normal equations, whose error would be
 * multiplied by the block's condition number) and its tile Cholesky as in an
 * LM step, a selected inverse over the factor's tiles (about two
 * factorizations' worth of tile products), then one small kernel per side
 * for the blocks.
 *
 * Valid after a completed arslam_lm_solve_loaded or arslam_lm_solve on the
 * handle, NO_CONVERGENCE included (the linearization at the returned point).
 * ARSLAM_E_STATE when no completed solve precedes the call or the last one
 * ended with rule EVAL_FAILED (both checked before any device call).
 * ARSLAM_E_UNSUPPORTED while arslam_lm_set_estimate_distortion is in effect
 * (checked first; arslam_lm_covariance_lens is the form that works under the
 * switch), with several ranks (arslam_lm_debug_force_multirank
 * included) and when the loaded problem's elimination_used is
 * ARSLAM_ELIM_MIXED; ARSLAM_ELIM_CAPTURES, _TAGS, and _AUTO or _MIXED
 * resolving to one whole side are supported (arslam_lm_covariance_anchored
 * is the form that works under a mixed set, with or without a call-time
 * anchor).  The call changes nothing a
 * later solve returns, repeated calls give the same bits, and nothing is
 * allocated or launched for it before the first call. */
#define ARSLAM_COV_OK 0
#define ARSLAM_COV_UNAVAILABLE 1     /* no covariance for this block: it is constant or unused */
#define ARSLAM_COV_RANK_DEFICIENT 2
typedef struct {
  int status;               /* ARSLAM_COV_OK or ARSLAM_COV_RANK_DEFICIENT for the whole problem */
  double min_pivot;         /* smallest squared pivot of the reduced system's real rows (1 with no
                               reduced system; -1 when the structural check or a pivot failed) */
  long n_reduced;           /* rows of the reduced system */
  long n_factor_tiles;      /* 64x64 tiles of its factor = tiles of the selected inverse */
  long n_factor_products;   /* 64x64x64 tile products of one factorization (updates, solves, diagonal tiles) */
  long n_selinv_products;   /* ... and of the selected inverse */
  double t_linearize_ms, t_factor_ms, t_selinv_ms, t_blocks_ms;   /* device times (HIP events): linearization,
                               reduced system + factorization, selected inverse, marginal blocks */
} arslam_lm_cov_info;
/* cov_cap [n_cap*36], cov_tag [n_tag*36], var_f [1], cap_status [n_cap],
 * tag_status [n_tag] (ARSLAM_COV_*), info: each nullable.  A block that is
 * constant or unused gets ARSLAM_COV_UNAVAILABLE and -1 in its 36 values (so
 * does var_f for a constant or unused camera); with info->status
 * RANK_DEFICIENT every value is -1 and every free block's status
 * RANK_DEFICIENT. */
int arslam_lm_covariance(arslam_lm *h, double *cov_cap, double *cov_tag, double *var_f, int *cap_status,
                         int *tag_status, arslam_lm_cov_info *info);
/* Covariance::GetCovarianceBlock(block, block, cov) for a block added through
 * arslam_lm_add_residual_block: 36 values for a pose block; 9 for the camera
 * block, var(f) at [0] and 0 elsewhere.  Computes on the first request after
 * a solve and serves later requests from the kept result.  *status (nullable)
 * = ARSLAM_COV_*; -1 in the values unless OK.  ARSLAM_E_INVALID_ARG for a
 * pointer that is not a block of the problem. */
int arslam_lm_covariance_block(arslam_lm *h, const double *block, double *cov, int *status);

/* ---- the same with the camera block whole: [f, l1, l2] ----
 * arslam_lm_covariance with cov_cam [9], the 3x3 marginal of the camera block
 * (row-major, [i][j] and [j][i] the same bits), and cam_status in place of
 * var_f.  It is not refused while arslam_lm_set_estimate_distortion is in
 * effect: H then runs over l1, l2 too (when the loaded problem has them live:
 * ARSLAM_CAMERA_RADIAL, the switch, a camera block that is not constant), the
 * capture and tag blocks are the marginals of that larger H -- wider, because
 * the lens is uncertain -- and the numeric test's min_pivot runs over the rows
 * of l1, l2 as well (same threshold).  With l1, l2 held (the switch off,
 * ARSLAM_CAMERA_PINHOLE, a constant camera) their rows and columns of cov_cam
 * are 0, [0] is var(f), and every other output is bit for bit what
 * arslam_lm_covariance returns on that handle (where that call is refused:
 * what it returns on a handle that never set the switch), by the same
 * launches.  A constant or unused camera: ARSLAM_COV_UNAVAILABLE and -1 in the
 * nine values.  Every other rule -- the point, apply_loss_function, no LM
 * diagonal, unit-variance residuals, the anchor's gauge, the structural check,
 * the refusals (several ranks, an unresolved ARSLAM_ELIM_MIXED, no completed
 * solve), what a later solve returns -- is arslam_lm_covariance's.  Nothing is
 * allocated for the live lens before the first _lens call on such a problem.
 * Each output nullable. */
int arslam_lm_covariance_lens(arslam_lm *h, double *cov_cap, double *cov_tag, double *cov_cam, int *cap_status,
                              int *tag_status, int *cam_status, arslam_lm_cov_info *info);
/* arslam_lm_covariance_block with the camera's 3x3 in the nine values of the
 * camera pointer.  Served from the kept result of an earlier _lens call. */
int arslam_lm_covariance_block_lens(arslam_lm *h, const double *block, double *cov, int *status);

/* ---- cross-covariance blocks (ceres::Covariance::Compute(pairs), GetCovarianceBlock(a, b)) ----
 * Block (a, b) of the same matrix C = H^-1 as arslam_lm_covariance: the same
 * free-parameter set, loss-corrected rows, no LM diagonal, unit-variance
 * residuals, at the point the last solve returned, in the gauge of whatever
 * the caller held constant.  What the marginals cannot give: how well tag j is
 * known relative to tag i (C_ii + C_jj - C_ij - C_ji over the translations), a
 * capture relative to the tags it saw, the focal against a pose.
 *
 * A block is {kind, index}: ARSLAM_BLOCK_CAMERA (index 0), _CAPTURE or _TAG
 * with the caller's index.  cov [n_pairs*36]: block (a, b) is rows of a by
 * columns of b, row-major, 6x6 for two poses ([t, w] each).  With the camera in
 * a pair the stride stays 36: for the focal against a pose, in either order,
 * the first 6 values are cov(f, pose) and the other 30 are 0; camera against
 * camera has var(f) at [0] and 0 elsewhere (l1 / l2 are held constant under
 * either camera model).
 *
 * status [n_pairs] (nullable): ARSLAM_COV_UNAVAILABLE, and -1 in the 36
 * values, if either block is constant or unused; ARSLAM_COV_RANK_DEFICIENT,
 * and -1, for every other pair when the problem is rank deficient (the
 * structural and numeric rule of arslam_lm_covariance, unchanged) or when an
 * eliminated block of the pair is itself singular; ARSLAM_COV_OK otherwise.
 * info (nullable) as in arslam_lm_covariance, except that n_selinv_products
 * counts the 64x64x64 tile products of the triangular solves below and
 * t_selinv_ms is their device time (t_blocks_ms: the right-hand sides and the
 * blocks).
 *
 * (a, b) and (b, a) are transposes of the same bits -- each unordered pair is
 * computed once, with a fixed choice of the side solved for, and transposed --
 * (a, a) is exactly symmetric, a pair listed twice and a repeated call give
 * the same bits, and a later solve returns what it would have returned without
 * the call.  (a, a) agrees with the marginal of arslam_lm_covariance to
 * rounding, not to the bit: the route differs.
 *
 * The device work: the linearization, reduced system and tile Cholesky of
 * arslam_lm_covariance, then, instead of the selected inverse (which holds
 * S^-1 only on the factor's tile pattern: two tags far apart under nested
 * dissection share no tile), a forward and a backward triangular solve of the
 * tile factor with six right-hand sides per distinct solved block, ten blocks
 * to a 64-column panel, level by level over the elimination tree; then one
 * wavefront per pair.  The panels go through in bounded batches, so device
 * memory does not grow with n_pairs beyond the 36 values per distinct pair.
 *
 * Preconditions and errors as arslam_lm_covariance: ARSLAM_E_STATE without a
 * completed solve, ARSLAM_E_UNSUPPORTED with several ranks, under
 * arslam_lm_set_estimate_distortion and under ARSLAM_ELIM_MIXED (so not for the SLAM mirror, which runs MIXED and holds no
 * block constant: arslam_lm_covariance_pairs_anchored is the form for it); an earlier arslam_lm_covariance call is neither needed nor
 * in the way.  ARSLAM_E_INVALID_ARG for a bad kind or index or n_pairs < 0;
 * n_pairs == 0 is OK.  Nothing is allocated or launched for this before its
 * first call. */
enum { ARSLAM_BLOCK_CAMERA = 0, ARSLAM_BLOCK_CAPTURE = 1, ARSLAM_BLOCK_TAG = 2 };
typedef struct { int kind_a, index_a, kind_b, index_b; } arslam_lm_cov_pair;
int arslam_lm_covariance_pairs(arslam_lm *h, const arslam_lm_cov_pair *pairs, int n_pairs,
                               double *cov /* [n_pairs*36] */, int *status /* [n_pairs], nullable */,
                               arslam_lm_cov_info *info /* nullable */);
/* Covariance::GetCovarianceBlock(block_a, block_b, cov) for blocks added
 * through arslam_lm_add_residual_block, in Ceres' shapes, row-major: 6x6 for
 * two poses; 3x6 for the camera against a pose (row 0 = cov(f, pose)), 6x3 for
 * a pose against the camera (column 0), 3x3 for the camera against itself
 * (var(f) at [0]); the l1 / l2 rows and columns are 0 (held constant), as in
 * arslam_lm_covariance_block.  Computes on every call.  *status (nullable) =
 * ARSLAM_COV_*; -1 in every value unless OK.  ARSLAM_E_INVALID_ARG for a
 * pointer that is not a block of the problem. */
int arslam_lm_covariance_block_pair(arslam_lm *h, const double *block_a, const double *block_b,
                                    double *cov, int *status);

/* arslam_lm_covariance_pairs over the matrix of arslam_lm_covariance_lens,
 * ARSLAM_BLOCK_CAMERA the 3-wide block [f, l1, l2], and not refused under
 * arslam_lm_set_estimate_distortion.  Still 36 values per pair, a 6x6
 * row-major: the camera as a fills rows 0..2 (cov(cam_i, b_j)), as b columns
 * 0..2, against itself the top-left 3x3; the rest is 0.  With l1, l2 held
 * their rows and columns are 0 and the values are arslam_lm_covariance_pairs'
 * bits (that call keeps a pose against the focal in its first six values;
 * this one in column 0, the transpose of (camera, pose)).  (a, b) and (b, a)
 * are transposes of the same bits.  Everything else as
 * arslam_lm_covariance_pairs. */
int arslam_lm_covariance_pairs_lens(arslam_lm *h, const arslam_lm_cov_pair *pairs, int n_pairs,
                                    double *cov /* [n_pairs*36] */, int *status /* [n_pairs], nullable */,
                                    arslam_lm_cov_info *info /* nullable */);
/* arslam_lm_covariance_block_pair over the same matrix, in Ceres' shapes: the
 * camera pointer's rows or columns are the three of [f, l1, l2]. */
int arslam_lm_covariance_block_pair_lens(arslam_lm *h, const double *block_a, const double *block_b,
                                         double *cov, int *status);

/* ---- covariance in a chosen anchor's gauge, under any e-block set ----
 * The _lens forms with one more pose block held fixed for the length of the
 * call: the anchor, a capture or a tag named by {anchor_kind, anchor_index}
 * (ARSLAM_BLOCK_CAPTURE or _TAG with the caller's index; ARSLAM_BLOCK_NONE:
 * the constant blocks alone) or by its pointer (NULL: none).  In Ceres' terms:
 * SetParameterBlockConstant(anchor), Covariance::Compute,
 * SetParameterBlockVariable(anchor) -- without touching the problem, so the
 * loaded problem, the handle's Jacobi scale and LM diagonal stay, and a later
 * solve returns the bits it would have returned without the call.
 *
 * H = J~'J~ is arslam_lm_covariance_lens' (loss-corrected rows at the point
 * the last solve returned, no LM diagonal, l1 and l2 live only when
 * estimated) with the anchor's six rows and columns deleted; C = H^-1 is the
 * covariance in that block's gauge, equal to what the same handle would return
 * at the same point had the block been constant.  The anchor's own status is
 * ARSLAM_COV_UNAVAILABLE with -1 in its values (so is a pair that names it),
 * the structural gauge check counts it as constant, and min_pivot leaves its
 * rows out.  An anchor that is already constant changes nothing.
 *
 * Unlike every form above these are not refused when elimination_used is
 * ARSLAM_ELIM_MIXED (Ceres' exact e-block set, what ARSLAM_ELIM_AUTO and the
 * SLAM mirror run), also after an append (ARSLAM_SETUP_APPEND): a mixed set's
 * direct groups -- residuals of two reduced blocks -- enter the reduced system
 * as their plain normal-equation blocks.  Several ranks stay
 * ARSLAM_E_UNSUPPORTED.  With an estimated lens they work on one whole side
 * (the load refuses a mixed set of both sides under the switch).
 *
 * Output shapes, the camera's 3x3 (three wide in a pair), nullability and the
 * error rules are the _lens forms'.  ARSLAM_E_INVALID_ARG for anchor_kind
 * ARSLAM_BLOCK_CAMERA (or any other value), an anchor_index out of range, or
 * an anchor pointer that is no pose block of the problem.  Repeated calls with
 * the same anchor give the same bits; (a, b) and (b, a) are transposes of the
 * same bits.  Nothing is allocated or launched for these forms before their
 * first call. */
#define ARSLAM_BLOCK_NONE (-1)
int arslam_lm_covariance_anchored(arslam_lm *h, int anchor_kind, int anchor_index, double *cov_cap,
                                  double *cov_tag, double *cov_cam /* [9] */, int *cap_status, int *tag_status,
                                  int *cam_status, arslam_lm_cov_info *info);
int arslam_lm_covariance_pairs_anchored(arslam_lm *h, int anchor_kind, int anchor_index,
                                        const arslam_lm_cov_pair *pairs, int n_pairs, double *cov, int *status,
                                        arslam_lm_cov_info *info);
/* arslam_lm_covariance_block_lens in the gauge of `anchor` (nullable).
 * Computes on the first request after a solve and serves later requests from
 * the kept result while the anchor is the same; another anchor recomputes. */
int arslam_lm_covariance_block_anchored(arslam_lm *h, const double *anchor, const double *block, double *cov,
                                        int *status);
/* arslam_lm_covariance_block_pair_lens in the gauge of `anchor` (nullable).
 * Computes on every call. */
int arslam_lm_covariance_block_pair_anchored(arslam_lm *h, const double *anchor, const double *block_a,
                                             const double *block_b, double *cov, int *status);

/* ---- Evaluate (ceres::Problem::Evaluate, Ceres 2.0, default EvaluateOptions) ----
 * The cost, the residuals, each residual block's loss weight and the gradient
 * at the values in the caller's memory at the time of the call, as Ceres reads
 * the user's pointers.  For residual block o, with r its 8 residuals and
 * s = |r|^2:
 *   residuals[8 o ..]  the corrected sqrt(rho'(s)) r (r itself without a loss)
 *   sq_norm[o]         s, uncorrected
 *   weight[o]          rho'(s); 1 for a block without a loss (a rejected
 *                      detection shows a weight near 0)
 *   *cost              1/2 sum rho(s) over all residual blocks
 *   gradient           J~'r~ over [camera 3 | captures 6 n_cap | tags 6 n_tag]
 *                      in the caller's indexing.  Exactly 0.0: the entries of
 *                      a constant block, of a block no residual block touches,
 *                      and l1, l2 unless the handle is ARSLAM_CAMERA_RADIAL with
 *                      estimate_distortion on and the camera free.
 * Every block's loss, its tag's side and the handle's camera model are
 * honoured.  apply_loss_function = 0: the plain r, 1/2 sum s and J'r, weights 1.
 * Every output is nullable; what is not asked for is not copied back.
 * A path of its own: it needs no prior solve, reads nothing of the solver's
 * state and leaves it untouched (a solve after it returns the bits of a solve
 * without it), and its results do not depend on options.elimination,
 * factor_executor or any other solver option.  The problem's structure goes
 * to the device at the first evaluate after a load or an added block; a call
 * then uploads the parameter values and runs three kernels.
 * ARSLAM_E_STATE: no problem loaded / no blocks.  ARSLAM_E_UNSUPPORTED: a
 * handle of several ranks (arslam_lm_debug_force_multirank included).  No
 * device: the failure arslam_lm_solve_loaded gives, never a CPU fallback. */
typedef struct {
  int apply_loss_function;   /* 1 */
} arslam_lm_evaluate_options;
int arslam_lm_evaluate_options_init(arslam_lm_evaluate_options *opt);
/* The problem loaded by arslam_lm_load_soa*, in that problem's observation
 * order (residuals[8 n_obs], sq_norm[n_obs], weight[n_obs],
 * gradient[3 + 6 n_cap + 6 n_tag]).  Reads the SoA arrays given at load time as
 * they are now: the results after a solve, the initial values before one,
 * anything the caller wrote to camera, cap or tag.  The problem's other arrays
 * (obs_cap, obs_tag, corners, the constant flags) must still be the loaded
 * ones: the first evaluate after a load reads them.  opt NULL: the defaults. */
int arslam_lm_evaluate(arslam_lm *h, const arslam_lm_evaluate_options *opt, double *cost, double *residuals,
                       double *sq_norm, double *weight, double *gradient);
/* The pointer-keyed residual blocks, in the order they were added, at the
 * values the caller's blocks hold now. */
int arslam_lm_evaluate_blocks(arslam_lm *h, const arslam_lm_evaluate_options *opt, double *cost, double *residuals,
                              double *sq_norm, double *weight);
/* A parameter block's 3 (camera) or 6 gradient entries from the last
 * arslam_lm_evaluate_blocks, as arslam_lm_covariance_block serves from a kept
 * result.  ARSLAM_E_STATE if there is none, or if the problem changed since
 * (a block added, a block set constant or variable, a reset). */
int arslam_lm_gradient_block(arslam_lm *h, const double *block, double *out);

/* Diagnostics */
int arslam_device_count(void);
const char *arslam_lm_last_error(void);
const char *arslam_lm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ARSLAM_LM_H */
