/*
 * arslam_localize.h -- C-ABI of the batched localizer: the reference's
 * ArSlamSolver::localizeMany (ar_slam_util.cpp:888-979) run for thousands of
 * queries at once on the device.
 *
 * Per query (localizeOne, :903-979):
 *   - find the first block of the capture whose tag was seen by a mapping
 *     capture (:911-927); none -> the query is skipped, pose untouched
 *     (:929-933);
 *   - initialise the capture pose from that block (initCapturePose, :943-947;
 *     ar_slam_util.cpp:98-115);
 *   - add every block of the capture as a residual with its tag held
 *     constant (:949-966) and the camera constant (:972);
 *   - ceres::Solve with the reference's options (optimize, :1001-1018): an
 *     independent Levenberg-Marquardt over the capture's 6 parameters, with
 *     its own trust region and termination.
 * With init_from_map = 0 the given pose is the initial value and no block is
 * required to be in the map (the plain optimize of a fixed map).
 *
 * Same conventions as arslam_lm.h: 0 or a negative ARSLAM_E_* code, no
 * exceptions across the ABI, handles not thread-safe.
 */
#ifndef ARSLAM_LOCALIZE_H
#define ARSLAM_LOCALIZE_H

#include "arslam_lm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ARSLAM_LOC_SKIPPED (-1)
#define ARSLAM_LOC_MAX_OBS 64   /* observations per query */

typedef struct {
  int n_query, n_tag, n_obs;
  const double *camera;               /* [3] intrinsics, constant (:972) */
  const double *tag;                  /* [n_tag*6] map tag poses, constant (:965) */
  const unsigned char *tag_in_map;    /* [n_tag] 1 if a mapping capture saw the tag; NULL = all */
  const int *query_start;             /* [n_query+1] observations of query q, in block order */
  const int *obs_tag;                 /* [n_obs] */
  const double *corners;              /* [n_obs*8] ArucoRect x0,y0,..,x3,y3 (centred px) */
  double *pose;                       /* [n_query*6] inv_pose t_c, w_c: in (init_from_map = 0), out */
  int init_from_map;                  /* 1: localizeOne's initialisation and skip rule */
} arslam_localize_batch;

typedef struct {
  int status;                  /* ARSLAM_CONVERGENCE / _NO_CONVERGENCE / _FAILURE or ARSLAM_LOC_SKIPPED */
  int rule;                    /* ARSLAM_RULE_* */
  int num_iterations;          /* Ceres summary.iterations.size() (iteration 0 included) */
  int num_successful_steps;
  int num_unsuccessful_steps;
  int init_obs;                /* observation used by initCapturePose, -1 if none */
  double initial_cost;
  double final_cost;
} arslam_localize_result;

/* One-shot: upload, solve every query, write poses back into b->pose and
 * one result per query into res (nullable). */
int arslam_localize_many(const arslam_localize_batch *b, const arslam_lm_options *opt,
                         arslam_localize_result *res);

/* Resident form (benchmarks, repeated localisation against one map). */
typedef struct arslam_localizer arslam_localizer;
int arslam_localizer_create(arslam_localizer **out, const arslam_lm_options *opt);
void arslam_localizer_destroy(arslam_localizer *h);
/* upload a batch (the map, the queries and their initial poses) */
int arslam_localizer_load(arslam_localizer *h, const arslam_localize_batch *b);
/* solve every loaded query from the loaded initial state; pose_out [n_query*6]
 * and res [n_query] are nullable (skip the download).  *kernel_ms (nullable)
 * receives the device time of the solve kernel. */
int arslam_localizer_solve(arslam_localizer *h, double *pose_out, arslam_localize_result *res,
                           double *kernel_ms);

/* ---- robust losses (arslam_lm.h ARSLAM_LOSS_*: Huber, SoftLOne, Cauchy) ----
 * One loss per observation (residual block), with the LM solver's and Ceres'
 * semantics (loss_function.cc, corrector.cc) -- what passing
 * `new ceres::CauchyLoss(a)` to AddResidualBlock at ar_slam_util.cpp:956-963
 * would do: s = |r|^2 over the block's 8 residuals, rows and Jacobian rows
 * times sqrt(rho'(s)), cost 1/2 sum rho(s); the Jacobi scaling, the LM
 * diagonal, the model cost change, the step quality and every termination
 * test work on the corrected quantities, and initial_cost / final_cost of
 * arslam_localize_result are the robust cost.  A batch whose observations
 * are all ARSLAM_LOSS_NONE runs the code without a loss (the same bits).
 *
 * An invalid kind, or a scale that is not finite and > 0 for a kind other
 * than NONE, returns ARSLAM_E_INVALID_ARG before any device call and leaves
 * the handle as it was. */

/* The default loss of every observation (initially NONE).  Takes effect at
 * the next solve; the loaded batch stays loaded. */
int arslam_localizer_set_loss(arslam_localizer *h, int kind, double a);
int arslam_localizer_get_loss(const arslam_localizer *h, int *kind, double *a);
/* arslam_localizer_load with the batch's own losses, obs_loss_kind and
 * obs_loss_a [n_obs] in observation order: they override the default for this
 * batch.  Both NULL = the default (arslam_localizer_load); exactly one NULL
 * is rejected. */
int arslam_localizer_load_loss(arslam_localizer *h, const arslam_localize_batch *b,
                               const unsigned char *obs_loss_kind, const double *obs_loss_a);
/* What the loss did, per observation, at the poses the last solve returned:
 * sq_residual = the plain s = |r|^2, weight = rho'(s) (1 without a loss; a
 * rejected detection shows a weight near 0).  Both -1 for the observations of
 * a skipped query.  [n_obs] each, either nullable.  ARSLAM_E_STATE before a
 * completed solve of the loaded batch. */
int arslam_localizer_observation_terms(arslam_localizer *h, double *sq_residual, double *weight);
/* arslam_localize_many with one loss for every observation. */
int arslam_localize_many_loss(const arslam_localize_batch *b, const arslam_lm_options *opt,
                              int kind, double a, arslam_localize_result *res);

/* ---- per-query pose covariance ----
 * What ceres::Covariance::Compute on the capture block after Solve would give
 * (Covariance::Options::apply_loss_function = true), for every query of the
 * batch at once.  At the pose the last solve returned, H = J~'J~ over the
 * query's 8k rows and its 6 parameters [t_c, w_c], the Jacobian rows corrected
 * by sqrt(rho'(s)) exactly as the solve corrects them (no LM diagonal, no
 * Jacobi scaling).  cov = H^-1, row-major 6x6 in the parameter order of
 * `pose`.  A query has no gauge freedom (tags and camera are constant), so
 * the inverse is well defined.
 *   - It assumes unit-variance residuals: with pixel noise sigma, multiply by
 *     sigma^2.
 *   - The camera centre in the world is -t_c, so the top-left 3x3 block is
 *     the covariance of its position.
 *   - The inverse is computed from the equilibrated matrix: c_j = 1/sqrt(H_jj),
 *     Hs = c H c (unit diagonal), Cholesky Hs = L L', C = c (L^-T L^-1) c.
 *     min_pivot = min_j L_jj^2, a scale-free number in (0, 1].
 *   - A query is rank deficient when some H_jj is not finite and > 0 or some
 *     squared pivot is not >= 1e-14 (a negative or NaN pivot included).  This
 *     stands where Ceres tests singular values against
 *     min_reciprocal_condition_number = 1e-14; it is NOT the same number (a
 *     pivot of the equilibrated Cholesky, not a ratio of singular values).
 *   - C[i][j] and C[j][i] are the same bits.
 *   - NO_CONVERGENCE and MIN_RADIUS queries get a covariance like any other:
 *     the linearization at the returned pose. */
/* cov_status: ARSLAM_COV_OK, _UNAVAILABLE, _RANK_DEFICIENT (arslam_lm.h).  UNAVAILABLE here: the query
 * was skipped, or its status is FAILURE with rule EVAL_FAILED, or the evaluation at the returned
 * pose is not finite. */
/* cov [n_query*36], cov_status [n_query] (ARSLAM_COV_*), min_pivot [n_query];
 * each nullable (all null: the call checks the state only).  For a status
 * other than OK all 36 values are -1; min_pivot is -1 for UNAVAILABLE and, for
 * RANK_DEFICIENT, the first offending pivot, or -1 when a diagonal entry
 * failed.  ARSLAM_E_STATE before a completed solve of the loaded batch
 * (checked before any device call).  Uses the losses the last solve used: a
 * set_loss after it changes nothing until the next solve.  Changes nothing
 * arslam_localizer_solve returns; repeated calls give the same bits. */
int arslam_localizer_covariance(arslam_localizer *h, double *cov, int *cov_status, double *min_pivot);
/* The same; *kernel_ms (nullable) receives the device time of the covariance
 * kernel, as arslam_localizer_solve's does for the solve (0 when nothing ran). */
int arslam_localizer_covariance_timed(arslam_localizer *h, double *cov, int *cov_status, double *min_pivot,
                                      double *kernel_ms);
/* arslam_localize_many_loss plus the covariances: cov [n_query*36] and
 * cov_status [n_query], either nullable. */
int arslam_localize_many_cov(const arslam_localize_batch *b, const arslam_lm_options *opt, int kind, double a,
                             arslam_localize_result *res, double *cov, int *cov_status);

/* ---- tag sides ----
 * A map tag carries its side length in metres (arslam_lm.h
 * ARSLAM_DEFAULT_TAG_SIZE and the rule for a valid side): it gives the tag's
 * constant world corners and initCapturePose's depth, local_z = focal * side /
 * sqrt(max_dist_sq).  The handle's default side holds for every tag of a batch
 * loaded afterwards without an array; the sides are bound at the load.  A batch
 * whose sides are all the default runs the code without sizes. */
int arslam_localizer_set_tag_size(arslam_localizer *h, double size);
int arslam_localizer_get_tag_size(const arslam_localizer *h, double *size);
/* arslam_localizer_load_loss with one side per map tag, tag_size [n_tag]
 * (NULL: the handle's default for every tag). */
int arslam_localizer_load_sized(arslam_localizer *h, const arslam_localize_batch *b, const double *tag_size,
                                const unsigned char *obs_loss_kind, const double *obs_loss_a);
/* arslam_localize_many_cov with one side per map tag (NULL: the default side). */
int arslam_localize_many_sized(const arslam_localize_batch *b, const arslam_lm_options *opt,
                               const double *tag_size, int kind, double a, arslam_localize_result *res,
                               double *cov, int *cov_status);

/* ---- camera model ----
 * The handle's camera model (arslam_lm.h ARSLAM_CAMERA_*), PINHOLE on creation.
 * Under RADIAL l1 = camera[1] and l2 = camera[2] of the loaded batch are a
 * known calibration, as the whole camera block is for the localizer.  The
 * model reaches arslam_localizer_load*, _solve, _observation_terms and
 * _covariance; the batch stays loaded when it changes, but the next
 * _observation_terms or _covariance needs a solve under the new model first
 * (ARSLAM_E_STATE).  init_from_map's initCapturePose stays the pinhole's: it
 * only seeds the LM.  An unknown value returns ARSLAM_E_INVALID_ARG and leaves
 * the handle unchanged.  The one-shot arslam_localize_many* calls have no
 * handle to set and stay PINHOLE. */
int arslam_localizer_set_camera_model(arslam_localizer *h, int model);
int arslam_localizer_camera_model(const arslam_localizer *h, int *model);

#ifdef __cplusplus
}
#endif
#endif
