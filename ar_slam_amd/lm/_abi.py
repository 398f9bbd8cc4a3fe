"""The C-ABI as ctypes: constants, the mirrors of the headers' structs, the one table of every
exported symbol's signature, the loaded library and the helpers every wrapper shares.

tests/test_boundary.py holds the table and the structs to include/*.h, prototype by prototype
and field by field; the headers are not read at import time (include/ need not be installed
beside the package).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # ar_slam_amd/, where the library is built
LIB_PATH = os.environ.get("ARSLAM_LIB") or os.path.join(HERE, "libarslam_lm.so")   # (override: variant builds)
MAX_ITERS = 1024
COMM_ID_BYTES = 128

TERMINATION = {0: "CONVERGENCE", 1: "NO_CONVERGENCE", 2: "FAILURE", 3: "USER_SUCCESS", 4: "USER_FAILURE"}
RULES = {0: "none", 1: "gradient_tolerance", 2: "parameter_tolerance", 3: "function_tolerance",
         4: "min_trust_region_radius", 5: "max_num_iterations", 6: "invalid_steps",
         7: "evaluation_failed", 8: "user_callback"}
ERRORS = {-1: "INVALID_ARG", -2: "UNSUPPORTED", -3: "NO_DEVICE", -4: "HIP", -5: "OUT_OF_MEMORY",
          -6: "COMM", -7: "STATE", -8: "DEVICE"}

SOLVER_CONTINUE, SOLVER_ABORT, SOLVER_TERMINATE_SUCCESSFULLY = 0, 1, 2
ELIM_AUTO, ELIM_CAPTURES, ELIM_TAGS, ELIM_MIXED = 0, 1, 2, 3   # arslam_lm_options.elimination
SETUP_LOAD, SETUP_VALUES, SETUP_APPEND = 0, 1, 2   # arslam_lm_summary.setup_kind
# ceres::LossFunction of a residual block (arslam_lm.h ARSLAM_LOSS_*); a loss is (kind, a)
LOSS_NONE, LOSS_HUBER, LOSS_SOFT_L_ONE, LOSS_CAUCHY = 0, 1, 2, 3
DEFAULT_TAG_SIZE = 0.0635   # arslam_lm.h ARSLAM_DEFAULT_TAG_SIZE: the side of a tag, metres
# the camera model of a handle (arslam_lm.h ARSLAM_CAMERA_*): the pinhole, or the radial model
# (u, v) = f d (x, y), d = 1 + r2 (l1 + l2 r2), with camera l1, l2 as a known calibration
# (or, on a mapper handle with set_estimate_distortion, as parameters of the solve)
CAMERA_PINHOLE, CAMERA_RADIAL = 0, 1
COV_OK, COV_UNAVAILABLE, COV_RANK_DEFICIENT = 0, 1, 2   # arslam_lm.h, arslam_localize.h ARSLAM_COV_*
BLOCK_CAMERA, BLOCK_CAPTURE, BLOCK_TAG = 0, 1, 2         # arslam_lm.h ARSLAM_BLOCK_* (covariance_pairs)
BLOCK_NONE = -1                                          # arslam_lm.h ARSLAM_BLOCK_NONE (no call-time anchor)
LOC_SKIPPED = -1                                         # arslam_localize.h ARSLAM_LOC_SKIPPED

P = C.POINTER
_i, _d, _l, _s, _vp = C.c_int, C.c_double, C.c_long, C.c_char_p, C.c_void_p
_dp, _ip, _up = P(C.c_double), P(C.c_int), P(C.c_ubyte)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int)


class LMError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"arslam_lm error {code} ({ERRORS.get(code, '?')}): {msg}")
        self.code = code


class _Struct(C.Structure):
    def to_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


# ---- include/arslam_lm.h ----

class Options(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double),
                ("initial_trust_region_radius", C.c_double),
                ("max_trust_region_radius", C.c_double),
                ("min_trust_region_radius", C.c_double),
                ("min_relative_decrease", C.c_double),
                ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
                ("max_num_consecutive_invalid_steps", C.c_int),
                ("jacobi_scaling", C.c_int), ("elimination", C.c_int),
                ("minimizer_progress_to_stdout", C.c_int),
                ("update_state_every_iteration", C.c_int),
                ("device", C.c_int), ("cholesky_skip_zero_tiles", C.c_int),
                ("reduced_ordering", C.c_int), ("kernel_timing", C.c_int), ("factor_executor", C.c_int),
                ("phase_timing", C.c_int)]


class Iteration(C.Structure):
    _fields_ = [("iteration", C.c_int),
                ("cost", C.c_double), ("cost_change", C.c_double),
                ("gradient_max_norm", C.c_double), ("gradient_norm", C.c_double),
                ("step_norm", C.c_double), ("relative_decrease", C.c_double),
                ("trust_region_radius", C.c_double),
                ("step_is_valid", C.c_int), ("step_is_successful", C.c_int),
                ("iteration_time", C.c_double), ("cumulative_time", C.c_double)]


ITER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, P(Iteration))


class Summary(C.Structure):
    _fields_ = [("termination", C.c_int), ("rule", C.c_int),
                ("num_successful_steps", C.c_int), ("num_unsuccessful_steps", C.c_int),
                ("num_linear_solves", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("fixed_cost", C.c_double), ("final_rms_px", C.c_double),
                ("n_obs", C.c_int), ("n_reduced", C.c_int),
                ("setup_time_s", C.c_double), ("setup_kind", C.c_int), ("minimizer_time_s", C.c_double),
                ("total_time_s", C.c_double),
                ("t_linearize_ms", C.c_double), ("t_schur_ms", C.c_double),
                ("t_cholesky_ms", C.c_double), ("t_solve_ms", C.c_double),
                ("t_backsub_ms", C.c_double), ("t_cost_ms", C.c_double),
                ("t_dominant_ms", C.c_double), ("dominant_flops", C.c_double),
                ("n_dominant_launches", C.c_long),
                ("n_factor_tiles", C.c_long), ("n_levels", C.c_int), ("n_update_tiles", C.c_long),
                ("factor_update_flops", C.c_double), ("factor_scalar_flops", C.c_double),
                ("comm_bytes", C.c_double),
                ("elimination_used", C.c_int), ("ceres_e_captures", C.c_int), ("ceres_e_tags", C.c_int),
                ("n_ranks", C.c_int), ("n_owned_captures", C.c_int), ("n_top_tiles", C.c_long),
                ("split_top_work", C.c_double), ("split_max_rank_work", C.c_double),
                ("split_total_work", C.c_double), ("t_factor_own_ms", C.c_double),
                ("t_factor_top_ms", C.c_double),
                ("n_iters", C.c_int), ("iters", Iteration * (MAX_ITERS + 1)),
                ("setup_phase_s", C.c_double * 5), ("comm_calls", C.c_long), ("n_active_ranks", C.c_int),
                ("order_reused", C.c_int)]

    def to_dict(self):
        its = [{f: getattr(self.iters[i], f) for f, _ in Iteration._fields_}
               for i in range(self.n_iters)]
        d = {f: getattr(self, f) for f, _ in Summary._fields_ if f not in ("iters", "termination", "rule")}
        d["setup_phase_s"] = list(self.setup_phase_s)
        d["termination"] = TERMINATION[self.termination]
        d["rule"] = RULES[self.rule]
        d["iterations"] = its
        return d


class SoaProblem(C.Structure):
    _fields_ = [("n_cap", C.c_int), ("n_tag", C.c_int), ("n_obs", C.c_int),
                ("camera", _dp), ("cap", _dp), ("tag", _dp),
                ("obs_cap", _ip), ("obs_tag", _ip), ("corners", _dp),
                ("camera_const", C.c_int), ("cap_const", _up), ("tag_const", _up)]


class CovInfo(_Struct):
    """arslam_lm_cov_info."""
    _fields_ = [("status", C.c_int), ("min_pivot", C.c_double), ("n_reduced", C.c_long),
                ("n_factor_tiles", C.c_long), ("n_factor_products", C.c_long), ("n_selinv_products", C.c_long),
                ("t_linearize_ms", C.c_double), ("t_factor_ms", C.c_double), ("t_selinv_ms", C.c_double),
                ("t_blocks_ms", C.c_double)]


class CovPair(C.Structure):
    """arslam_lm_cov_pair: a row of the (n, 4) int32 array covariance_pairs passes."""
    _fields_ = [("kind_a", C.c_int), ("index_a", C.c_int), ("kind_b", C.c_int), ("index_b", C.c_int)]


class EvaluateOptions(C.Structure):
    """arslam_lm_evaluate_options."""
    _fields_ = [("apply_loss_function", C.c_int)]


# ---- include/arslam_lm_debug.h ----

class TilePlanFacts(C.Structure):
    _fields_ = [("tiles_per_side", C.c_int), ("n_assembled", C.c_long), ("n_tiles", C.c_long),
                ("n_levels", C.c_int), ("n_split", C.c_long), ("n_dag_tasks", C.c_long),
                ("fill_first_ok", C.c_int), ("phase_split", C.c_long), ("grid", C.c_int * 2),
                ("n_cont_tasks", C.c_long), ("dag_valid", C.c_int)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["grid"] = tuple(self.grid)
        return d


class StepInfo(_Struct):
    """arslam_lm_step_info."""
    _fields_ = [("n", C.c_long), ("n_cap", C.c_int), ("n_tag", C.c_int), ("n_reduced", C.c_long),
                ("n_padded", C.c_long), ("cam_row", C.c_int), ("elimination_used", C.c_int), ("n_groups", C.c_int),
                ("n_direct", C.c_int), ("n_big_groups", C.c_int), ("n_chunk_groups", C.c_int),
                ("n_split_dest", C.c_int), ("max_contrib", C.c_int), ("n_tiles", C.c_long),
                ("n_assembled_tiles", C.c_long), ("cost", C.c_double), ("fixed_cost", C.c_double),
                ("model_cost_change", C.c_double), ("candidate_cost", C.c_double),
                ("candidate_fixed_cost", C.c_double), ("e_step2", C.c_double), ("f_step2", C.c_double),
                ("e_step_bad", C.c_int), ("candidate_bad", C.c_int), ("f_step_bad", C.c_int), ("indefinite", C.c_int)]


class PlanInfo(_Struct):
    _fields_ = [("n_reduced", C.c_long), ("n_padded", C.c_long), ("pad_rows", C.c_long),
                ("tiles_per_side", C.c_int), ("n_parts", C.c_int), ("camera_row", C.c_int),
                ("n_levels", C.c_int), ("n_assembled_tiles", C.c_long), ("n_factor_tiles", C.c_long),
                ("n_update_tiles", C.c_long), ("n_update_items", C.c_long), ("n_split_targets", C.c_long),
                ("update_flops", C.c_double), ("n_dag_tasks", C.c_long), ("dag_valid", C.c_int),
                ("factor_flops", C.c_double), ("scalar_flops", C.c_double), ("fill_first_ok", C.c_int)]


class OrderStep(_Struct):
    _fields_ = [("side", C.c_int), ("order_reused", C.c_int), ("recomputed", C.c_int), ("etree_height", C.c_int),
                ("pad_rows", C.c_long)]


class SplitInfo(_Struct):
    _fields_ = [("tiles_per_side", C.c_int), ("n_top_cols", C.c_int), ("n_own_cols", C.c_int),
                ("n_top_tiles", C.c_long), ("n_tiles", C.c_long), ("n_dag_tasks", C.c_long),
                ("phase_split", C.c_long), ("dag_valid", C.c_int), ("n_owned_captures", C.c_int),
                ("top_work", C.c_double), ("max_rank_work", C.c_double), ("total_work", C.c_double),
                ("n_active", C.c_int)]


# ---- include/arslam_localize.h ----

class LocalizeBatchC(C.Structure):
    _fields_ = [("n_query", C.c_int), ("n_tag", C.c_int), ("n_obs", C.c_int),
                ("camera", _dp), ("tag", _dp), ("tag_in_map", _up), ("query_start", _ip),
                ("obs_tag", _ip), ("corners", _dp), ("pose", _dp), ("init_from_map", C.c_int)]


class LocalizeResult(C.Structure):
    _fields_ = [("status", C.c_int), ("rule", C.c_int), ("num_iterations", C.c_int),
                ("num_successful_steps", C.c_int), ("num_unsuccessful_steps", C.c_int),
                ("init_obs", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double)]


# ---- include/arslam_slam.h ----

class Transform(C.Structure):
    _fields_ = [("child_frame_id", C.c_char * 128), ("translation", C.c_double * 3),
                ("rotation", C.c_double * 4)]


# Every symbol the four headers declare and its argtypes, in the headers' order.  The two comm ids
# are c_char_p where the header has unsigned char[128], because callers pass bytes.
SIGNATURES = {
    # ---- include/arslam_lm.h ----
    "arslam_lm_options_init": [P(Options)],
    "arslam_lm_create": [P(_vp), P(Options)],
    "arslam_lm_destroy": [_vp],
    "arslam_lm_set_options": [_vp, P(Options)],
    "arslam_lm_get_options": [_vp, P(Options)],
    "arslam_lm_add_residual_block": [_vp, _dp, _dp, _dp, _dp],
    "arslam_lm_set_loss": [_vp, _i, _d],
    "arslam_lm_get_loss": [_vp, _ip, _dp],
    "arslam_lm_add_residual_block_loss": [_vp, _dp, _dp, _dp, _dp, _i, _d],
    "arslam_lm_set_tag_size": [_vp, _d],
    "arslam_lm_get_tag_size": [_vp, _dp],
    "arslam_lm_set_camera_model": [_vp, _i],
    "arslam_lm_camera_model": [_vp, _ip],
    "arslam_lm_set_estimate_distortion": [_vp, _i],
    "arslam_lm_estimate_distortion": [_vp, _ip],
    "arslam_lm_add_residual_block_sized": [_vp, _dp, _dp, _dp, _dp, _d, _i, _d],
    "arslam_lm_set_parameter_block_constant": [_vp, _dp],
    "arslam_lm_set_parameter_block_variable": [_vp, _dp],
    "arslam_lm_solve": [_vp, P(Summary)],
    "arslam_lm_reset": [_vp],
    "arslam_lm_num_residual_blocks": [_vp],
    "arslam_lm_load_soa": [_vp, P(SoaProblem)],
    "arslam_lm_solve_loaded": [_vp, P(Summary)],
    "arslam_lm_load_soa_loss": [_vp, P(SoaProblem), _up, _dp],
    "arslam_lm_load_soa_sized": [_vp, P(SoaProblem), _dp, _up, _dp],
    "arslam_lm_solve_soa": [P(SoaProblem), P(Options), P(Summary)],
    "arslam_comm_unique_id": [_s],
    "arslam_lm_set_comm": [_vp, _i, _i, _s],
    "arslam_lm_set_comm_callback": [_vp, _i, _i, ALLREDUCE_FN, _vp],
    "arslam_lm_owned_captures": [_vp, _ip, _i, _ip],
    "arslam_lm_set_iteration_callback": [_vp, ITER_CB, _vp],
    "arslam_lm_covariance": [_vp, _dp, _dp, _dp, _ip, _ip, P(CovInfo)],
    "arslam_lm_covariance_block": [_vp, _dp, _dp, _ip],
    "arslam_lm_covariance_lens": [_vp, _dp, _dp, _dp, _ip, _ip, _ip, P(CovInfo)],
    "arslam_lm_covariance_block_lens": [_vp, _dp, _dp, _ip],
    "arslam_lm_covariance_pairs": [_vp, P(CovPair), _i, _dp, _ip, P(CovInfo)],
    "arslam_lm_covariance_block_pair": [_vp, _dp, _dp, _dp, _ip],
    "arslam_lm_covariance_pairs_lens": [_vp, P(CovPair), _i, _dp, _ip, P(CovInfo)],
    "arslam_lm_covariance_block_pair_lens": [_vp, _dp, _dp, _dp, _ip],
    "arslam_lm_covariance_anchored": [_vp, _i, _i, _dp, _dp, _dp, _ip, _ip, _ip, P(CovInfo)],
    "arslam_lm_covariance_pairs_anchored": [_vp, _i, _i, P(CovPair), _i, _dp, _ip, P(CovInfo)],
    "arslam_lm_covariance_block_anchored": [_vp, _dp, _dp, _dp, _ip],
    "arslam_lm_covariance_block_pair_anchored": [_vp, _dp, _dp, _dp, _dp, _ip],
    "arslam_lm_evaluate_options_init": [P(EvaluateOptions)],
    "arslam_lm_evaluate": [_vp, P(EvaluateOptions), _dp, _dp, _dp, _dp, _dp],
    "arslam_lm_evaluate_blocks": [_vp, P(EvaluateOptions), _dp, _dp, _dp, _dp],
    "arslam_lm_gradient_block": [_vp, _dp, _dp],
    "arslam_device_count": [],
    "arslam_lm_last_error": [],
    "arslam_lm_version": [],
    # ---- include/arslam_lm_debug.h ----
    "arslam_debug_residual_jacobian": [_i, _dp, _dp, _dp, _dp, _dp, _dp],
    "arslam_debug_residual_jacobian_sized": [_i, _dp, _dp, _dp, _dp, _dp, _dp, _dp],
    "arslam_debug_residual_jacobian_model": [_i, _i, _dp, _dp, _dp, _dp, _dp, _dp, _dp],
    "arslam_debug_residual_jacobian_distortion": [_i, _dp, _dp, _dp, _dp, _dp, _dp, _dp],
    "arslam_debug_residual_jacobian_loss": [_i, _dp, _dp, _dp, _dp, _up, _dp, _dp, _dp, _dp],
    "arslam_debug_angle_axis_rotate": [_i, _dp, _dp, _dp, _ip],
    "arslam_debug_dense_llt": [_l, _dp, _dp, _dp, _ip],
    "arslam_debug_dense_llt_ex": [_l, _dp, _dp, _dp, _ip, _i],
    "arslam_debug_tile_llt": [_l, _dp, _dp, _up, _i, _up, C.c_uint, _dp, _dp, _up, _ip, P(TilePlanFacts)],
    "arslam_debug_tile_plan": [_i, _up, _up, _up, P(TilePlanFacts)],
    "arslam_debug_selinv": [_l, _dp, _up, _dp, _up, _ip],
    "arslam_debug_tile_solve": [_l, _dp, _up, _i, _dp, _dp, _ip],
    "arslam_lm_debug_reduced_rows": [_vp, _ip, _ip, _ip],
    "arslam_lm_debug_camera_rows": [_vp, _d, _l, _dp, _ip],
    "arslam_lm_debug_cov_camera_rows": [_vp, _l, _dp, _ip],
    "arslam_lm_debug_step_stages": [_vp, _d, P(StepInfo), _dp, _dp, _dp, _dp, _dp, _ip, _dp, _dp],
    "arslam_lm_debug_step_stages_sharded": [_vp, _d, _i, P(StepInfo), _ip, _dp, _dp, _dp, _dp, _up, _dp, _ip, _ip, _dp,
                                            _dp],
    "arslam_lm_debug_evaluate_times": [_vp, _dp],
    "arslam_debug_schur_stamps": [P(C.c_ulonglong)],
    "arslam_lm_debug_force_indefinite": [_vp, C.c_ulonglong],
    "arslam_lm_debug_break_dependency": [_vp, _l, P(_l)],
    "arslam_lm_debug_force_multirank": [_vp, _i],
    "arslam_lm_debug_tag_pair_tile": [_vp, _dp, _dp, _ip],
    "arslam_debug_ceres_e_blocks": [P(SoaProblem), _ip],
    "arslam_debug_mixed_groups": [P(SoaProblem), _ip, _up, _up],
    "arslam_debug_reduced_plan": [P(SoaProblem), _i, _i, P(PlanInfo), _ip],
    "arslam_debug_reduced_plan_side": [P(SoaProblem), _i, P(PlanInfo)],
    "arslam_debug_order_memory": [P(SoaProblem), _i, _i, _i, _up, P(OrderStep), P(_ip), P(_ip)],
    "arslam_debug_dag_simulate": [P(SoaProblem), _i, C.c_uint, _i, _ip],
    "arslam_debug_dag_simulate_started": [P(SoaProblem), _i, _i, C.c_uint, _i, _ip],
    "arslam_debug_dag_workgroup_limit": [_i],
    "arslam_debug_dag_fault_detail": [P(SoaProblem), _ip, _s, _i],
    "arslam_debug_box_fingerprint": [_i, _dp],
    "arslam_debug_rank_split": [P(SoaProblem), _i, _i, P(SplitInfo), _ip],
    "arslam_debug_dag_tasks": [P(SoaProblem), _i, _i, _ip, _ip, _l, P(_l), _ip],
    "arslam_debug_gather_extend": [P(SoaProblem), _i, _ip, _ip],
    "arslam_debug_schur_store_table": [_i, _ip, _up],
    # ---- include/arslam_localize.h ----
    "arslam_localize_many": [P(LocalizeBatchC), P(Options), P(LocalizeResult)],
    "arslam_localizer_create": [P(_vp), P(Options)],
    "arslam_localizer_destroy": [_vp],
    "arslam_localizer_load": [_vp, P(LocalizeBatchC)],
    "arslam_localizer_solve": [_vp, _dp, P(LocalizeResult), _dp],
    "arslam_localizer_set_loss": [_vp, _i, _d],
    "arslam_localizer_get_loss": [_vp, _ip, _dp],
    "arslam_localizer_load_loss": [_vp, P(LocalizeBatchC), _up, _dp],
    "arslam_localizer_observation_terms": [_vp, _dp, _dp],
    "arslam_localize_many_loss": [P(LocalizeBatchC), P(Options), _i, _d, P(LocalizeResult)],
    "arslam_localizer_covariance": [_vp, _dp, _ip, _dp],
    "arslam_localizer_covariance_timed": [_vp, _dp, _ip, _dp, _dp],
    "arslam_localize_many_cov": [P(LocalizeBatchC), P(Options), _i, _d, P(LocalizeResult), _dp, _ip],
    "arslam_localizer_set_tag_size": [_vp, _d],
    "arslam_localizer_get_tag_size": [_vp, _dp],
    "arslam_localizer_load_sized": [_vp, P(LocalizeBatchC), _dp, _up, _dp],
    "arslam_localize_many_sized": [P(LocalizeBatchC), P(Options), _dp, _i, _d, P(LocalizeResult), _dp, _ip],
    "arslam_localizer_set_camera_model": [_vp, _i],
    "arslam_localizer_camera_model": [_vp, _ip],
    # ---- include/arslam_slam.h ----
    "arslam_slam_create": [P(_vp), P(Options)],
    "arslam_slam_destroy": [_vp],
    "arslam_slam_set_verbose": [_vp, _i],
    "arslam_slam_set_loss": [_vp, _i, _d],
    "arslam_slam_set_localize_loss": [_vp, _i, _d],
    "arslam_slam_set_default_aruco_size": [_vp, _d],
    "arslam_slam_set_aruco_size": [_vp, _s, _d],
    "arslam_slam_aruco_size": [_vp, _i, _dp],
    "arslam_slam_debug_init_pose": [_i, _dp, _dp, _dp, _d, _dp],
    "arslam_slam_set_camera_model": [_vp, _i],
    "arslam_slam_camera_model": [_vp, _ip],
    "arslam_slam_camera_distortion": [_vp, _dp],
    "arslam_slam_load_yaml": [_vp, _s],
    "arslam_slam_load_yaml_string": [_vp, _s],
    "arslam_slam_save_yaml": [_vp, _s],
    "arslam_slam_add_detections": [_vp, _s, _i, _i, _s, _i, P(_s), _dp, _ip],
    "arslam_slam_solve": [_vp],
    "arslam_slam_solve_incremental": [_vp],
    "arslam_slam_localize_many": [_vp, _i],
    "arslam_slam_localize_covariance": [_vp, _i, _dp, _ip],
    "arslam_slam_covariance": [_vp, _i, P(CovInfo)],
    "arslam_slam_aruco_covariance": [_vp, _i, _dp, _ip],
    "arslam_slam_capture_covariance": [_vp, _i, _dp, _ip],
    "arslam_slam_camera_covariance": [_vp, _dp, _ip],
    "arslam_slam_covariance_pair": [_vp, _i, _i, _i, _i, _i, _dp, _ip],
    "arslam_slam_evaluate": [_vp, _dp, _dp, _dp],
    "arslam_slam_num_captures": [_vp],
    "arslam_slam_num_arucos": [_vp],
    "arslam_slam_num_blocks": [_vp],
    "arslam_slam_num_solves": [_vp],
    "arslam_slam_last_summary": [_vp, P(Summary)],
    "arslam_slam_solve_summary": [_vp, _i, P(Summary)],
    "arslam_slam_solve_capture": [_vp, _i, _ip],
    "arslam_slam_unsolved_captures": [_vp, _ip, _i, _ip],
    "arslam_slam_capture": [_vp, _i, _s, _i, _dp],
    "arslam_slam_set_capture_pose": [_vp, _i, _dp],
    "arslam_slam_aruco": [_vp, _i, _s, _i, _dp, _ip],
    "arslam_slam_set_aruco_pose": [_vp, _i, _dp],
    "arslam_slam_block": [_vp, _i, _ip, _ip, _dp, _ip],
    "arslam_slam_camera": [_vp, _dp, _ip, _ip],
    "arslam_slam_set_camera": [_vp, _dp],
    "arslam_slam_get_transforms": [_vp, P(Transform), _i, _ip],
    "arslam_slam_camera_info": [_vp, _dp, _dp],
}
# what a symbol returns where that is not the int status
RESTYPES = {"arslam_lm_destroy": None, "arslam_localizer_destroy": None, "arslam_slam_destroy": None,
            "arslam_lm_last_error": C.c_char_p, "arslam_lm_version": C.c_char_p}
EXPORTS = list(SIGNATURES)


def apply_signatures(L):
    """Type every symbol of the table that L has; one it lacks is skipped (a variant build from an
    earlier tree, under the ARSLAM_LIB A/B) and fails as an AttributeError where it is called."""
    for name, argtypes in SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.argtypes = argtypes
            fn.restype = RESTYPES.get(name, C.c_int)
    return L


_lib = None


def library_path():
    return LIB_PATH


def library_info():
    """Which library this process measures: its file, the sha256 of the file (first 12 hex) and the
    build it reports (commit + source digest, ar_slam_amd/build.py build_id)."""
    import hashlib
    with open(LIB_PATH, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()[:12]
    v = lib().arslam_lm_version().decode()
    return {"file": os.path.basename(LIB_PATH), "sha256": sha, "version": v.split(" build ")[0],
            "build": v.split(" build ")[-1] if " build " in v else "unknown"}


def lib():
    """Load the HIP library (fails loudly when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -m ar_slam_amd.build` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        _lib = apply_signatures(C.CDLL(LIB_PATH))
    return _lib


def _check(rc):
    if rc != 0:
        raise LMError(rc, lib().arslam_lm_last_error().decode(errors="replace"))


def device_count():
    return lib().arslam_device_count()


def make_options(**kw):
    o = Options()
    lib().arslam_lm_options_init(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(f"unknown solver option {k}")
        setattr(o, k, v)
    return o


class _Owner:
    """A handle of the library in ``_h``: made by the entry point ``_create`` names under the solver
    options `opts`, freed by the one ``_destroy`` names on close() or collection."""
    _create = _destroy = None

    def __init__(self, **opts):
        self._h = C.c_void_p()
        _check(getattr(lib(), self._create)(C.byref(self._h), C.byref(make_options(**opts))))

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


_POINTER_OF = {np.dtype(np.float64): _dp, np.dtype(np.int32): _ip, np.dtype(np.uint8): _up}


def _ptr(a, to=None):
    """The ctypes pointer to a numpy array's data -- double*, int* or unsigned char* by its dtype,
    or the type `to` -- and None for None (a nullable argument left out)."""
    return None if a is None else a.ctypes.data_as(to or _POINTER_OF[a.dtype])


def _per(value, n):
    """value broadcast to a contiguous float64 [n]: one per tag or observation, or a scalar for all."""
    return _f64(np.broadcast_to(np.asarray(value, np.float64), (n,)))


def _obs_loss(obs_loss, n_obs):
    """obs_loss = (kinds[n_obs], a[n_obs]) as the uint8 and float64 arrays a load takes; (None, None)
    for None."""
    if obs_loss is None:
        return None, None
    kinds = np.ascontiguousarray(obs_loss[0], np.uint8).reshape(-1)
    scales = _f64(obs_loss[1]).reshape(-1)
    if kinds.shape[0] != n_obs or scales.shape[0] != n_obs:
        raise ValueError("obs_loss: one kind and one scale per observation")
    return kinds, scales


def _load(h, batch, n_tag, n_obs, tag_size, obs_loss, plain, with_loss, sized):
    """Load `batch` (an arslam_soa_problem or arslam_localize_batch) into handle h through the entry
    point the arguments ask for: `sized` with tag_size, else `with_loss` with obs_loss, else `plain`."""
    kinds, scales = _obs_loss(obs_loss, n_obs)
    if tag_size is not None:
        _check(sized(h, C.byref(batch), _ptr(_per(tag_size, n_tag)), _ptr(kinds), _ptr(scales)))
    elif obs_loss is None:
        _check(plain(h, C.byref(batch)))
    else:
        _check(with_loss(h, C.byref(batch), _ptr(kinds), _ptr(scales)))
