"""Python binding of libarslam_lm.so (ctypes over the C-ABI in include/arslam_lm.h).

This is the host-side mirror of the reference's solver interface used by the
tests, the benchmark and smoke():

* :class:`Problem` mirrors ``ceres::Problem`` as ArSlamSolver drives it --
  ``add_residual_block(corners, camera, capture, tag)`` is
  ``AddResidualBlock(AutoDiff<ArucoReprojectionError,8,3,6,6>, nullptr,
  camera, capture, aruco)`` (ar_slam_util.cpp:720-727),
  ``set_parameter_block_constant`` is ``SetParameterBlockConstant``
  (:965, :972) and ``solve`` is ``ceres::Solve`` (:1015); parameter blocks
  are caller-owned float64 numpy arrays updated in place.
* :func:`solve_soa` / :class:`ResidentProblem` are the bulk struct-of-arrays
  path (problem uploaded once to HBM, solved many times).

There is no CPU fallback: if the HIP library is missing or no GPU is
present, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ARSLAM_LIB") or os.path.join(HERE, "libarslam_lm.so")   # (override: variant builds)
MAX_ITERS = 1024
COMM_ID_BYTES = 128

TERMINATION = {0: "CONVERGENCE", 1: "NO_CONVERGENCE", 2: "FAILURE", 3: "USER_SUCCESS", 4: "USER_FAILURE"}
RULES = {0: "none", 1: "gradient_tolerance", 2: "parameter_tolerance", 3: "function_tolerance",
         4: "min_trust_region_radius", 5: "max_num_iterations", 6: "invalid_steps",
         7: "evaluation_failed", 8: "user_callback"}
ERRORS = {-1: "INVALID_ARG", -2: "UNSUPPORTED", -3: "NO_DEVICE", -4: "HIP", -5: "OUT_OF_MEMORY",
          -6: "COMM", -7: "STATE", -8: "DEVICE"}

# Every symbol include/arslam_lm.h declares (checked by the CPU tests).
EXPORTS = ["arslam_lm_options_init", "arslam_lm_create", "arslam_lm_destroy",
           "arslam_lm_set_options", "arslam_lm_get_options",
           "arslam_lm_add_residual_block", "arslam_lm_set_parameter_block_constant",
           "arslam_lm_set_parameter_block_variable", "arslam_lm_solve", "arslam_lm_reset",
           "arslam_lm_num_residual_blocks", "arslam_lm_load_soa", "arslam_lm_solve_loaded",
           "arslam_lm_solve_soa", "arslam_comm_unique_id", "arslam_lm_set_comm", "arslam_lm_set_comm_callback",
           "arslam_device_count", "arslam_lm_last_error", "arslam_lm_version",
           "arslam_lm_set_iteration_callback", "arslam_lm_owned_captures",
           "arslam_lm_set_loss", "arslam_lm_get_loss", "arslam_lm_add_residual_block_loss",
           "arslam_lm_load_soa_loss", "arslam_debug_residual_jacobian_loss", "arslam_slam_set_loss",
           "arslam_lm_set_tag_size", "arslam_lm_get_tag_size", "arslam_lm_add_residual_block_sized",
           "arslam_lm_load_soa_sized", "arslam_debug_residual_jacobian_sized",
           "arslam_localizer_set_tag_size", "arslam_localizer_get_tag_size", "arslam_localizer_load_sized",
           "arslam_localize_many_sized",
           "arslam_slam_debug_init_pose", "arslam_slam_set_default_aruco_size", "arslam_slam_set_aruco_size", "arslam_slam_aruco_size",
           "arslam_lm_set_camera_model", "arslam_lm_camera_model", "arslam_debug_residual_jacobian_model",
           "arslam_localizer_set_camera_model", "arslam_localizer_camera_model",
           "arslam_slam_set_camera_model", "arslam_slam_camera_model", "arslam_slam_camera_distortion",
           "arslam_lm_set_estimate_distortion", "arslam_lm_estimate_distortion",
           "arslam_debug_residual_jacobian_distortion", "arslam_lm_debug_camera_rows",
           "arslam_lm_debug_step_stages",
           "arslam_lm_evaluate_options_init", "arslam_lm_evaluate", "arslam_lm_evaluate_blocks",
           "arslam_lm_gradient_block", "arslam_slam_evaluate", "arslam_lm_debug_evaluate_times",
           "arslam_debug_residual_jacobian", "arslam_debug_dense_llt", "arslam_debug_dense_llt_ex",
           "arslam_debug_tile_llt", "arslam_debug_tile_plan",
           "arslam_debug_angle_axis_rotate", "arslam_debug_selinv", "arslam_lm_debug_force_indefinite",
           "arslam_lm_covariance", "arslam_lm_covariance_block", "arslam_lm_debug_reduced_rows",
           "arslam_lm_covariance_pairs", "arslam_lm_covariance_block_pair", "arslam_debug_tile_solve",
           "arslam_lm_covariance_lens", "arslam_lm_covariance_block_lens", "arslam_lm_covariance_pairs_lens",
           "arslam_lm_covariance_block_pair_lens", "arslam_lm_debug_cov_camera_rows",
           "arslam_lm_debug_force_multirank", "arslam_lm_debug_break_dependency", "arslam_lm_debug_tag_pair_tile",
           "arslam_debug_reduced_plan", "arslam_debug_reduced_plan_side", "arslam_debug_schur_stamps", "arslam_debug_ceres_e_blocks",
           "arslam_debug_order_memory",
           "arslam_debug_mixed_groups",
           "arslam_debug_dag_simulate", "arslam_debug_dag_simulate_started", "arslam_debug_dag_workgroup_limit",
           "arslam_debug_dag_fault_detail", "arslam_debug_box_fingerprint",
           "arslam_debug_rank_split", "arslam_debug_gather_extend", "arslam_debug_schur_store_table",
           "arslam_debug_dag_tasks",
           "arslam_localize_many", "arslam_localizer_create", "arslam_localizer_destroy",
           "arslam_localizer_load", "arslam_localizer_solve",
           "arslam_localizer_set_loss", "arslam_localizer_get_loss", "arslam_localizer_load_loss",
           "arslam_localizer_observation_terms", "arslam_localize_many_loss", "arslam_slam_set_localize_loss",
           "arslam_localizer_covariance", "arslam_localizer_covariance_timed", "arslam_localize_many_cov",
           "arslam_slam_localize_covariance",
           "arslam_slam_create", "arslam_slam_destroy", "arslam_slam_set_verbose", "arslam_slam_load_yaml",
           "arslam_slam_load_yaml_string", "arslam_slam_save_yaml", "arslam_slam_add_detections",
           "arslam_slam_solve", "arslam_slam_solve_incremental", "arslam_slam_localize_many",
           "arslam_slam_num_captures", "arslam_slam_num_arucos", "arslam_slam_num_blocks",
           "arslam_slam_num_solves", "arslam_slam_last_summary", "arslam_slam_solve_summary",
           "arslam_slam_solve_capture", "arslam_slam_unsolved_captures", "arslam_slam_capture", "arslam_slam_set_capture_pose", "arslam_slam_aruco", "arslam_slam_set_aruco_pose",
           "arslam_slam_block", "arslam_slam_camera", "arslam_slam_set_camera",
           "arslam_slam_get_transforms", "arslam_slam_camera_info"]

_dp = C.POINTER(C.c_double)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int)
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
_ip = C.POINTER(C.c_int)
_up = C.POINTER(C.c_ubyte)


class LMError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"arslam_lm error {code} ({ERRORS.get(code, '?')}): {msg}")
        self.code = code


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


ITER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(Iteration))


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


COV_OK, COV_UNAVAILABLE, COV_RANK_DEFICIENT = 0, 1, 2   # arslam_lm.h ARSLAM_COV_*
BLOCK_CAMERA, BLOCK_CAPTURE, BLOCK_TAG = 0, 1, 2         # arslam_lm.h ARSLAM_BLOCK_* (covariance_pairs)


class CovInfo(C.Structure):
    """arslam_lm_cov_info."""
    _fields_ = [("status", C.c_int), ("min_pivot", C.c_double), ("n_reduced", C.c_long),
                ("n_factor_tiles", C.c_long), ("n_factor_products", C.c_long), ("n_selinv_products", C.c_long),
                ("t_linearize_ms", C.c_double), ("t_factor_ms", C.c_double), ("t_selinv_ms", C.c_double),
                ("t_blocks_ms", C.c_double)]

    def to_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class StepInfo(C.Structure):
    """arslam_lm_step_info (include/arslam_lm_debug.h)."""
    _fields_ = [("n", C.c_long), ("n_cap", C.c_int), ("n_tag", C.c_int), ("n_reduced", C.c_long),
                ("n_padded", C.c_long), ("cam_row", C.c_int), ("elimination_used", C.c_int), ("n_groups", C.c_int),
                ("n_direct", C.c_int), ("n_big_groups", C.c_int), ("n_chunk_groups", C.c_int),
                ("n_split_dest", C.c_int), ("max_contrib", C.c_int), ("n_tiles", C.c_long),
                ("n_assembled_tiles", C.c_long), ("cost", C.c_double), ("fixed_cost", C.c_double),
                ("model_cost_change", C.c_double), ("candidate_cost", C.c_double),
                ("candidate_fixed_cost", C.c_double), ("e_step2", C.c_double), ("f_step2", C.c_double),
                ("e_step_bad", C.c_int), ("candidate_bad", C.c_int), ("f_step_bad", C.c_int), ("indefinite", C.c_int)]

    def to_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class EvaluateOptions(C.Structure):
    """arslam_lm_evaluate_options."""
    _fields_ = [("apply_loss_function", C.c_int)]


class SoaProblem(C.Structure):
    _fields_ = [("n_cap", C.c_int), ("n_tag", C.c_int), ("n_obs", C.c_int),
                ("camera", _dp), ("cap", _dp), ("tag", _dp),
                ("obs_cap", _ip), ("obs_tag", _ip), ("corners", _dp),
                ("camera_const", C.c_int), ("cap_const", _up), ("tag_const", _up)]


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
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m ar_slam_amd.build` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    L.arslam_lm_options_init.argtypes = [C.POINTER(Options)]
    L.arslam_lm_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Options)]
    L.arslam_lm_set_comm_callback.argtypes = [C.c_void_p, C.c_int, C.c_int, ALLREDUCE_FN, C.c_void_p]
    L.arslam_lm_set_options.argtypes = [C.c_void_p, C.POINTER(Options)]
    L.arslam_debug_rank_split.argtypes = [C.POINTER(SoaProblem), C.c_int, C.c_int, C.POINTER(SplitInfo), _ip]
    L.arslam_lm_owned_captures.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    for fn in ("arslam_slam_destroy", "arslam_slam_set_verbose", "arslam_slam_load_yaml",
               "arslam_slam_load_yaml_string", "arslam_slam_save_yaml", "arslam_slam_add_detections",
               "arslam_slam_solve", "arslam_slam_solve_incremental", "arslam_slam_localize_many",
               "arslam_slam_num_captures", "arslam_slam_num_arucos", "arslam_slam_num_blocks",
               "arslam_slam_num_solves", "arslam_slam_last_summary", "arslam_slam_solve_summary",
               "arslam_slam_solve_capture", "arslam_slam_unsolved_captures", "arslam_slam_capture",
               "arslam_slam_set_capture_pose", "arslam_slam_aruco", "arslam_slam_set_aruco_pose",
               "arslam_slam_block", "arslam_slam_camera", "arslam_slam_set_camera",
               "arslam_slam_get_transforms", "arslam_slam_camera_info"):
        getattr(L, fn).argtypes = None
    L.arslam_slam_destroy.restype = None
    L.arslam_slam_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Options)]
    L.arslam_localize_many.argtypes = [C.POINTER(LocalizeBatchC), C.POINTER(Options), C.POINTER(LocalizeResult)]
    L.arslam_localizer_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Options)]
    L.arslam_localizer_destroy.argtypes = [C.c_void_p]
    L.arslam_localizer_destroy.restype = None
    L.arslam_localizer_load.argtypes = [C.c_void_p, C.POINTER(LocalizeBatchC)]
    L.arslam_localizer_solve.argtypes = [C.c_void_p, _dp, C.POINTER(LocalizeResult), C.POINTER(C.c_double)]
    L.arslam_lm_get_options.argtypes = [C.c_void_p, C.POINTER(Options)]
    L.arslam_lm_destroy.argtypes = [C.c_void_p]
    L.arslam_lm_destroy.restype = None
    L.arslam_lm_add_residual_block.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
    if hasattr(L, "arslam_lm_set_loss"):   # (absent from older variant builds under A/B)
        L.arslam_lm_add_residual_block_loss.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, C.c_int, C.c_double]
        L.arslam_lm_set_loss.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.arslam_lm_get_loss.argtypes = [C.c_void_p, _ip, _dp]
        L.arslam_lm_load_soa_loss.argtypes = [C.c_void_p, C.POINTER(SoaProblem), _up, _dp]
        L.arslam_debug_residual_jacobian_loss.argtypes = [C.c_int, _dp, _dp, _dp, _dp, _up, _dp, _dp, _dp, _dp]
        L.arslam_slam_set_loss.argtypes = [C.c_void_p, C.c_int, C.c_double]
    if hasattr(L, "arslam_localizer_set_loss"):   # (likewise)
        L.arslam_localizer_set_loss.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.arslam_localizer_get_loss.argtypes = [C.c_void_p, _ip, _dp]
        L.arslam_localizer_load_loss.argtypes = [C.c_void_p, C.POINTER(LocalizeBatchC), _up, _dp]
        L.arslam_localizer_observation_terms.argtypes = [C.c_void_p, _dp, _dp]
        L.arslam_localize_many_loss.argtypes = [C.POINTER(LocalizeBatchC), C.POINTER(Options), C.c_int, C.c_double,
                                                C.POINTER(LocalizeResult)]
        L.arslam_slam_set_localize_loss.argtypes = [C.c_void_p, C.c_int, C.c_double]
    if hasattr(L, "arslam_localizer_covariance"):   # (likewise)
        L.arslam_localizer_covariance.argtypes = [C.c_void_p, _dp, _ip, _dp]
        L.arslam_localizer_covariance_timed.argtypes = [C.c_void_p, _dp, _ip, _dp, _dp]
        L.arslam_localize_many_cov.argtypes = [C.POINTER(LocalizeBatchC), C.POINTER(Options), C.c_int, C.c_double,
                                               C.POINTER(LocalizeResult), _dp, _ip]
        L.arslam_slam_localize_covariance.argtypes = [C.c_void_p, C.c_int, _dp, _ip]
    if hasattr(L, "arslam_lm_set_tag_size"):
        L.arslam_lm_set_tag_size.argtypes = [C.c_void_p, C.c_double]
        L.arslam_lm_get_tag_size.argtypes = [C.c_void_p, _dp]
        L.arslam_lm_add_residual_block_sized.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, C.c_double, C.c_int,
                                                         C.c_double]
        L.arslam_lm_load_soa_sized.argtypes = [C.c_void_p, C.POINTER(SoaProblem), _dp, _up, _dp]
        L.arslam_debug_residual_jacobian_sized.argtypes = [C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
        L.arslam_localizer_set_tag_size.argtypes = [C.c_void_p, C.c_double]
        L.arslam_localizer_get_tag_size.argtypes = [C.c_void_p, _dp]
        L.arslam_localizer_load_sized.argtypes = [C.c_void_p, C.POINTER(LocalizeBatchC), _dp, _up, _dp]
        L.arslam_localize_many_sized.argtypes = [C.POINTER(LocalizeBatchC), C.POINTER(Options), _dp, C.c_int,
                                                 C.c_double, C.POINTER(LocalizeResult), _dp, _ip]
        L.arslam_slam_set_default_aruco_size.argtypes = [C.c_void_p, C.c_double]
        L.arslam_slam_set_aruco_size.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        L.arslam_slam_aruco_size.argtypes = [C.c_void_p, C.c_int, _dp]
        L.arslam_slam_debug_init_pose.argtypes = [C.c_int, _dp, _dp, _dp, C.c_double, _dp]
    if hasattr(L, "arslam_lm_set_camera_model"):   # (absent from older variant builds under A/B)
        L.arslam_lm_set_camera_model.argtypes = [C.c_void_p, C.c_int]
        L.arslam_lm_camera_model.argtypes = [C.c_void_p, _ip]
        L.arslam_debug_residual_jacobian_model.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
        L.arslam_localizer_set_camera_model.argtypes = [C.c_void_p, C.c_int]
        L.arslam_localizer_camera_model.argtypes = [C.c_void_p, _ip]
        L.arslam_slam_set_camera_model.argtypes = [C.c_void_p, C.c_int]
        L.arslam_slam_camera_model.argtypes = [C.c_void_p, _ip]
        L.arslam_slam_camera_distortion.argtypes = [C.c_void_p, _dp]
    if hasattr(L, "arslam_lm_set_estimate_distortion"):   # (absent from older variant builds under A/B)
        L.arslam_lm_set_estimate_distortion.argtypes = [C.c_void_p, C.c_int]
        L.arslam_lm_estimate_distortion.argtypes = [C.c_void_p, _ip]
        L.arslam_debug_residual_jacobian_distortion.argtypes = [C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
        L.arslam_lm_debug_camera_rows.argtypes = [C.c_void_p, C.c_double, C.c_long, _dp, _ip]
    if hasattr(L, "arslam_lm_debug_step_stages"):   # (likewise)
        L.arslam_lm_debug_step_stages.argtypes = [C.c_void_p, C.c_double, C.POINTER(StepInfo), _dp, _dp, _dp, _dp, _dp,
                                                  _ip, _dp, _dp]
    if hasattr(L, "arslam_lm_evaluate"):   # (absent from older variant builds under A/B)
        L.arslam_lm_evaluate_options_init.argtypes = [C.POINTER(EvaluateOptions)]
        L.arslam_lm_evaluate.argtypes = [C.c_void_p, C.POINTER(EvaluateOptions), _dp, _dp, _dp, _dp, _dp]
        L.arslam_lm_evaluate_blocks.argtypes = [C.c_void_p, C.POINTER(EvaluateOptions), _dp, _dp, _dp, _dp]
        L.arslam_lm_gradient_block.argtypes = [C.c_void_p, _dp, _dp]
        L.arslam_slam_evaluate.argtypes = [C.c_void_p, _dp, _dp, _dp]
        L.arslam_lm_debug_evaluate_times.argtypes = [C.c_void_p, _dp]
    L.arslam_lm_set_parameter_block_constant.argtypes = [C.c_void_p, _dp]
    L.arslam_lm_set_parameter_block_variable.argtypes = [C.c_void_p, _dp]
    L.arslam_lm_solve.argtypes = [C.c_void_p, C.POINTER(Summary)]
    L.arslam_lm_reset.argtypes = [C.c_void_p]
    L.arslam_lm_num_residual_blocks.argtypes = [C.c_void_p]
    L.arslam_lm_load_soa.argtypes = [C.c_void_p, C.POINTER(SoaProblem)]
    L.arslam_lm_solve_loaded.argtypes = [C.c_void_p, C.POINTER(Summary)]
    L.arslam_lm_solve_soa.argtypes = [C.POINTER(SoaProblem), C.POINTER(Options), C.POINTER(Summary)]
    L.arslam_comm_unique_id.argtypes = [C.c_char_p]
    L.arslam_lm_set_comm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p]
    L.arslam_device_count.argtypes = []
    L.arslam_lm_last_error.restype = C.c_char_p
    L.arslam_lm_version.restype = C.c_char_p
    L.arslam_debug_residual_jacobian.argtypes = [C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]
    L.arslam_debug_dense_llt.argtypes = [C.c_long, _dp, _dp, _dp, C.POINTER(C.c_int)]
    L.arslam_debug_angle_axis_rotate.argtypes = [C.c_int, _dp, _dp, _dp, _ip]
    L.arslam_debug_selinv.argtypes = [C.c_long, _dp, _up, _dp, _up, _ip]
    if hasattr(L, "arslam_debug_tile_llt"):   # (absent from older variant builds under A/B)
        L.arslam_debug_tile_llt.argtypes = [C.c_long, _dp, _dp, _up, C.c_int, _up, C.c_uint, _dp, _dp, _up, _ip,
                                            C.c_void_p]
        L.arslam_debug_tile_plan.argtypes = [C.c_int, _up, _up, _up, C.c_void_p]
    L.arslam_lm_covariance.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip, _ip, C.POINTER(CovInfo)]
    L.arslam_lm_covariance_block.argtypes = [C.c_void_p, _dp, _dp, _ip]
    L.arslam_lm_covariance_pairs.argtypes = [C.c_void_p, _ip, C.c_int, _dp, _ip, C.POINTER(CovInfo)]
    L.arslam_lm_covariance_block_pair.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip]
    if hasattr(L, "arslam_lm_covariance_lens"):   # (absent from older variant builds under A/B)
        L.arslam_lm_covariance_lens.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip, _ip, _ip, C.POINTER(CovInfo)]
        L.arslam_lm_covariance_block_lens.argtypes = [C.c_void_p, _dp, _dp, _ip]
        L.arslam_lm_covariance_pairs_lens.argtypes = [C.c_void_p, _ip, C.c_int, _dp, _ip, C.POINTER(CovInfo)]
        L.arslam_lm_covariance_block_pair_lens.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip]
        L.arslam_lm_debug_cov_camera_rows.argtypes = [C.c_void_p, C.c_long, _dp, _ip]
    L.arslam_debug_tile_solve.argtypes = [C.c_long, _dp, _up, C.c_int, _dp, _dp, _ip]
    L.arslam_lm_debug_reduced_rows.argtypes = [C.c_void_p, _ip, _ip, _ip]
    L.arslam_debug_ceres_e_blocks.argtypes = [C.POINTER(SoaProblem), _ip]
    L.arslam_debug_mixed_groups.argtypes = [C.POINTER(SoaProblem), _ip, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]
    L.arslam_lm_debug_force_indefinite.argtypes = [C.c_void_p, C.c_ulonglong]
    L.arslam_lm_debug_force_multirank.argtypes = [C.c_void_p, C.c_int]
    L.arslam_debug_dag_workgroup_limit.argtypes = [C.c_int]
    L.arslam_lm_set_iteration_callback.argtypes = [C.c_void_p, ITER_CB, C.c_void_p]
    L.arslam_lm_debug_break_dependency.argtypes = [C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    if hasattr(L, "arslam_lm_debug_tag_pair_tile"):   # (absent from older variant builds under A/B)
        L.arslam_lm_debug_tag_pair_tile.argtypes = [C.c_void_p, _dp, _dp, C.POINTER(C.c_int)]
    if hasattr(L, "arslam_debug_schur_store_table"):   # (likewise)
        L.arslam_debug_schur_store_table.argtypes = [C.c_int, _ip, C.POINTER(C.c_ubyte)]
    if hasattr(L, "arslam_debug_dag_tasks"):   # (likewise)
        L.arslam_debug_dag_tasks.argtypes = [C.POINTER(SoaProblem), C.c_int, C.c_int, _ip, _ip, C.c_long,
                                             C.POINTER(C.c_long), _ip]
    _lib = L
    return L


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


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


class _Soa:
    def __init__(self, camera, cap, tag, obs_cap, obs_tag, corners, camera_const=False,
                 cap_const=None, tag_const=None):
        self.camera = _f64(camera).copy()
        self.cap = _f64(cap, (-1, 6)).copy()
        self.tag = _f64(tag, (-1, 6)).copy()
        self.obs_cap = np.ascontiguousarray(obs_cap, np.int32)
        self.obs_tag = np.ascontiguousarray(obs_tag, np.int32)
        self.corners = _f64(corners, (-1, 8))
        self.cap_const = None if cap_const is None else np.ascontiguousarray(cap_const, np.uint8)
        self.tag_const = None if tag_const is None else np.ascontiguousarray(tag_const, np.uint8)
        self.s = SoaProblem(self.cap.shape[0], self.tag.shape[0], self.obs_cap.shape[0],
                            self.camera.ctypes.data_as(_dp), self.cap.ctypes.data_as(_dp),
                            self.tag.ctypes.data_as(_dp), self.obs_cap.ctypes.data_as(_ip),
                            self.obs_tag.ctypes.data_as(_ip), self.corners.ctypes.data_as(_dp),
                            int(bool(camera_const)),
                            None if self.cap_const is None else self.cap_const.ctypes.data_as(_up),
                            None if self.tag_const is None else self.tag_const.ctypes.data_as(_up))


def solve_soa(camera, cap, tag, obs_cap, obs_tag, corners, camera_const=False, cap_const=None,
              tag_const=None, loss=None, obs_loss=None, **opts):
    """One-shot bulk solve.  Returns (camera, cap, tag, summary dict).
    loss = (kind, a): every observation's robust loss; obs_loss = (kinds[n_obs], a[n_obs]): one per
    observation (see ResidentProblem)."""
    if loss is not None or obs_loss is not None:
        R = ResidentProblem(camera, cap, tag, obs_cap, obs_tag, corners, camera_const, cap_const, tag_const,
                            loss=loss, obs_loss=obs_loss, **opts)
        try:
            s = R.solve()
            return R.camera, R.cap, R.tag, s
        finally:
            R.close()
    A = _Soa(camera, cap, tag, obs_cap, obs_tag, corners, camera_const, cap_const, tag_const)
    s = Summary()
    _check(lib().arslam_lm_solve_soa(C.byref(A.s), C.byref(make_options(**opts)), C.byref(s)))
    return A.camera, A.cap, A.tag, s.to_dict()


def warm_up(device=0):
    """One small solve (the 'tiny' synthetic graph) on `device`: the process's one-time runtime
    start (the library's code objects loaded on first launch, its stream, page-locked buffers),
    which a first load would otherwise carry.  Returns its wall time (s)."""
    import time
    from . import synth
    t = time.perf_counter()
    g = synth.config_graph("tiny")
    ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, device=device).solve()
    return time.perf_counter() - t


def solve_graph(g, loss=None, obs_loss=None, **opts):
    return solve_soa(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, loss=loss, obs_loss=obs_loss, **opts)


class _Handle:
    def __init__(self, **opts):
        self._h = C.c_void_p()
        _check(lib().arslam_lm_create(C.byref(self._h), C.byref(make_options(**opts))))

    def close(self):
        if self._h:
            lib().arslam_lm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_options(self, **opts):
        _check(lib().arslam_lm_set_options(self._h, C.byref(make_options(**opts))))

    def get_options(self) -> Options:
        o = Options()
        _check(lib().arslam_lm_get_options(self._h, C.byref(o)))
        return o

    def set_loss(self, kind, a=0.0):
        """The handle's default loss (LOSS_*, scale a): what add_residual_block gives the blocks
        added afterwards and a bulk load gives every observation.  Drops a loaded SoA problem."""
        _check(lib().arslam_lm_set_loss(self._h, int(kind), float(a)))

    def get_loss(self):
        """(kind, a) of the default loss."""
        k, a = C.c_int(0), C.c_double(0.0)
        _check(lib().arslam_lm_get_loss(self._h, C.byref(k), C.byref(a)))
        return k.value, a.value

    def set_tag_size(self, size):
        """The handle's default tag side in metres (DEFAULT_TAG_SIZE on creation): what
        add_residual_block gives the blocks added afterwards and a bulk load gives every tag.
        Drops a loaded SoA problem."""
        _check(lib().arslam_lm_set_tag_size(self._h, float(size)))

    def get_tag_size(self):
        s = C.c_double(0.0)
        _check(lib().arslam_lm_get_tag_size(self._h, C.byref(s)))
        return s.value

    def set_camera_model(self, model):
        """The handle's camera model, CAMERA_PINHOLE (on creation) or CAMERA_RADIAL: under RADIAL
        the camera block's l1, l2 are a known calibration the solve holds.  Drops a loaded problem
        and a kept covariance; the next load or solve uses it."""
        _check(lib().arslam_lm_set_camera_model(self._h, int(model)))

    def camera_model(self):
        m = C.c_int(0)
        _check(lib().arslam_lm_camera_model(self._h, C.byref(m)))
        return m.value

    def set_estimate_distortion(self, on=True):
        """Estimate the distortion (off on creation): under CAMERA_RADIAL, with the camera block not
        constant, l1 and l2 are parameters like f and camera[1], camera[2] come back estimated;
        ignored under CAMERA_PINHOLE.  Drops a loaded problem and a kept covariance.  While it is in
        effect several ranks, ELIM_MIXED on a set that mixes sides and the covariances whose camera
        output is one scalar are refused (UNSUPPORTED); ``covariance_lens`` and the other ``_lens``
        forms carry the camera block whole and work."""
        _check(lib().arslam_lm_set_estimate_distortion(self._h, int(on)))

    def estimate_distortion(self):
        v = C.c_int(0)
        _check(lib().arslam_lm_estimate_distortion(self._h, C.byref(v)))
        return bool(v.value)

    def set_iteration_callback(self, fn):
        """ceres::IterationCallback: fn(iteration dict) -> SOLVER_CONTINUE / SOLVER_ABORT /
        SOLVER_TERMINATE_SUCCESSFULLY (None = continue); fn=None removes it."""
        if fn is None:
            self._iter_cb = None
            _check(lib().arslam_lm_set_iteration_callback(self._h, C.cast(None, ITER_CB), None))
            return

        def tramp(ctx, it):
            try:
                d = {f: getattr(it.contents, f) for f, _ in Iteration._fields_}
                r = fn(d)
                return SOLVER_CONTINUE if r is None else int(r)
            except Exception:   # noqa: BLE001 -- a raising callback aborts the solve
                return SOLVER_ABORT
        self._iter_cb = ITER_CB(tramp)
        _check(lib().arslam_lm_set_iteration_callback(self._h, self._iter_cb, None))

    def debug_force_indefinite(self, step_mask):
        """Test hook: linear solves whose bit min(i,63) is set in step_mask see an indefinite
        reduced system (camera diagonal -1), i.e. an invalid LM step."""
        _check(lib().arslam_lm_debug_force_indefinite(self._h, C.c_ulonglong(step_mask & (2**64 - 1))))

    def debug_force_multirank(self, on=True):
        """Test hook: the multi-rank path (split, two-phase factorization, every collective) with
        one rank, so set_comm(0, 1, uid) makes a one-rank RCCL communicator on a one-GPU box."""
        _check(lib().arslam_lm_debug_force_multirank(self._h, 1 if on else 0))

    def debug_evaluate_times(self):
        """The last evaluate()'s device times under phase_timing=1, ms: {upload, k_eval_obs,
        k_eval_blocks, k_eval_tree, copy_back} (arslam_lm_debug_evaluate_times)."""
        ms = np.zeros(5)
        _check(lib().arslam_lm_debug_evaluate_times(self._h, ms.ctypes.data_as(_dp)))
        return dict(zip(("upload", "k_eval_obs", "k_eval_blocks", "k_eval_tree", "copy_back"), ms.tolist()))

    def debug_step_stages(self, radius):
        """Every stage of one LM step of the loaded problem at its loaded point under `radius`
        (arslam_lm_debug_step_stages): a dict of the arslam_lm_step_info fields and
        ``g``, ``colnorm``, ``scale``, ``diag``, ``xc`` (n,) by the caller's slots; ``S``
        (n_reduced, n_reduced) the assembled system before the factorization, ``rhs``
        (n_reduced,) its right-hand side row, ``S_padded`` (n_padded, n_padded) every row of the
        padded system; ``row_slot`` (n_reduced,) the caller's slot of a row, -1 for padding; ``y``
        (n_reduced,) the reduced solution."""
        info = StepInfo()
        L = lib()
        _check(L.arslam_lm_debug_step_stages(self._h, float(radius), C.byref(info), None, None, None, None, None,
                                             None, None, None))
        n, nR, N = info.n, info.n_reduced, info.n_padded
        v = {k: np.zeros(n) for k in ("g", "colnorm", "scale", "diag", "xc")}
        S = np.zeros((max(N, 1), max(N, 1)))
        slot = np.zeros(max(nR, 1), np.int32)
        y = np.zeros(max(nR, 1))
        _check(L.arslam_lm_debug_step_stages(self._h, float(radius), C.byref(info), v["g"].ctypes.data_as(_dp),
                                             v["colnorm"].ctypes.data_as(_dp), v["scale"].ctypes.data_as(_dp),
                                             v["diag"].ctypes.data_as(_dp), S.ctypes.data_as(_dp),
                                             slot.ctypes.data_as(_ip), y.ctypes.data_as(_dp),
                                             v["xc"].ctypes.data_as(_dp)))
        out = info.to_dict()
        out.update(v)
        S = S[:N, :N]
        out.update(S_padded=S, S=S[:nR, :nR].copy(), rhs=S[nR, :nR].copy() if N else np.zeros(0),
                   row_slot=slot[:nR], y=y[:nR])
        return out

    def set_comm(self, rank, nranks, uid):
        """Join the ranks' exchange: ``uid`` is an RCCL unique id (bytes, one GPU per
        rank) or a host all-reduce ``fn(array, op)`` reducing a numpy array in place
        (op "sum" or "max"), e.g. over torch.distributed gloo."""
        if callable(uid):
            fn = uid

            def tramp(ctx, buf, count, dtype, op):
                try:
                    ct = C.c_double if dtype == 0 else C.c_ubyte
                    arr = np.ctypeslib.as_array(C.cast(buf, C.POINTER(ct)), shape=(count,))
                    fn(arr, "sum" if op == 0 else "max")
                    return 0
                except Exception:   # noqa: BLE001 -- reported to the solver as a comm failure
                    return 1
            self._comm_cb = ALLREDUCE_FN(tramp)
            _check(lib().arslam_lm_set_comm_callback(self._h, rank, nranks, self._comm_cb, None))
        else:
            _check(lib().arslam_lm_set_comm(self._h, rank, nranks, uid))


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().arslam_comm_unique_id(buf))
    return buf.raw


def _evaluate(call, n_cap, n_tag, n_obs, apply_loss, residuals, gradient):
    """One arslam_lm_evaluate / _evaluate_blocks call (call(opt, cost, residuals, sq_norm, weight[,
    gradient])) into fresh arrays; the result dict of ResidentProblem.evaluate."""
    o = EvaluateOptions(1 if apply_loss else 0)
    cost = C.c_double(0.0)
    res = np.zeros((n_obs, 8)) if residuals else None
    sq = np.zeros(n_obs)
    w = np.zeros(n_obs)
    args = [C.byref(o), C.byref(cost), res.ctypes.data_as(_dp) if residuals else None, sq.ctypes.data_as(_dp),
            w.ctypes.data_as(_dp)]
    out = {"cost": 0.0, "residuals": res, "sq_norm": sq, "weight": w, "gradient": None}
    if gradient is not None:
        g = np.zeros(3 + 6 * n_cap + 6 * n_tag) if gradient else None
        args.append(g.ctypes.data_as(_dp) if gradient else None)
        if gradient:
            out["gradient"] = {"camera": g[:3], "cap": g[3:3 + 6 * n_cap].reshape(n_cap, 6),
                               "tag": g[3 + 6 * n_cap:].reshape(n_tag, 6)}
    _check(call(*args))
    out["cost"] = cost.value
    return out


class ResidentProblem(_Handle):
    """SoA problem uploaded once to HBM; ``solve()`` restarts from the loaded state."""

    def __init__(self, camera, cap, tag, obs_cap, obs_tag, corners, camera_const=False,
                 cap_const=None, tag_const=None, comm=None, force_multirank=False, loss=None, obs_loss=None,
                 tag_size=None, camera_model=None, estimate_distortion=None, **opts):
        """loss = (kind, a): the robust loss of every observation (the handle's default loss);
        obs_loss = (kinds[n_obs], a[n_obs]): one loss per observation, in observation order;
        tag_size = [n_tag] the tags' sides in metres (a scalar: every tag's); None: DEFAULT_TAG_SIZE;
        camera_model = CAMERA_PINHOLE / CAMERA_RADIAL (None: the handle's, PINHOLE);
        estimate_distortion = True: under CAMERA_RADIAL l1, l2 are estimated (set_estimate_distortion)."""
        super().__init__(**opts)
        if camera_model is not None:
            self.set_camera_model(camera_model)
        if estimate_distortion is not None:
            self.set_estimate_distortion(estimate_distortion)
        if force_multirank:
            self.debug_force_multirank(True)
        if comm is not None:
            self.set_comm(*comm)
        if loss is not None:
            self.set_loss(*loss)
        self.A = _Soa(camera, cap, tag, obs_cap, obs_tag, corners, camera_const, cap_const, tag_const)
        kinds = scales = None
        if obs_loss is not None:
            kinds = np.ascontiguousarray(obs_loss[0], np.uint8).reshape(-1)
            scales = _f64(obs_loss[1]).reshape(-1)
            if kinds.shape[0] != self.A.s.n_obs or scales.shape[0] != self.A.s.n_obs:
                raise ValueError("obs_loss: one kind and one scale per observation")
        if tag_size is not None:
            sizes = _f64(np.broadcast_to(np.asarray(tag_size, np.float64), (self.A.s.n_tag,)))
            _check(lib().arslam_lm_load_soa_sized(self._h, C.byref(self.A.s), sizes.ctypes.data_as(_dp),
                                                  kinds.ctypes.data_as(_up) if kinds is not None else None,
                                                  scales.ctypes.data_as(_dp) if scales is not None else None))
        elif obs_loss is None:
            _check(lib().arslam_lm_load_soa(self._h, C.byref(self.A.s)))
        else:
            _check(lib().arslam_lm_load_soa_loss(self._h, C.byref(self.A.s), kinds.ctypes.data_as(_up),
                                                 scales.ctypes.data_as(_dp)))

    def solve(self):
        s = Summary()
        _check(lib().arslam_lm_solve_loaded(self._h, C.byref(s)))
        return s.to_dict()

    def evaluate(self, apply_loss=True, residuals=True, gradient=True):
        """ceres::Problem::Evaluate at the values ``camera`` / ``cap`` / ``tag`` hold now (the results
        after a solve, the loaded values before one, anything written there): ``cost`` = 1/2 sum rho,
        ``residuals`` (n_obs, 8) corrected by sqrt(rho'), ``sq_norm`` (n_obs,) the uncorrected |r|^2,
        ``weight`` (n_obs,) rho' (1 without a loss; near 0 for a rejected detection) and ``gradient``
        {camera (3,), cap (n_cap, 6), tag (n_tag, 6)}, exactly 0 for constant and unseen blocks
        (arslam_lm_evaluate).  apply_loss=False: the plain r, 1/2 sum s and J'r.  residuals / gradient
        False: that output is not computed back (its key is None)."""
        n_cap, n_tag, n_obs = self.A.s.n_cap, self.A.s.n_tag, self.A.s.n_obs
        return _evaluate(lambda *a: lib().arslam_lm_evaluate(self._h, *a), n_cap, n_tag, n_obs, apply_loss, residuals,
                         gradient)

    def covariance(self):
        """Marginal covariances at the point the last ``solve()`` returned (arslam_lm_covariance):
        ``cap`` (n_cap, 6, 6), ``tag`` (n_tag, 6, 6), ``var_f``, ``cap_status`` / ``tag_status``
        (COV_*) and ``info`` (arslam_lm_cov_info as a dict).  Unit-variance residuals: times sigma^2."""
        n_cap, n_tag = self.A.s.n_cap, self.A.s.n_tag
        cap = np.zeros((n_cap, 6, 6))
        tag = np.zeros((n_tag, 6, 6))
        var_f = C.c_double(0.0)
        cs = np.zeros(max(n_cap, 1), np.int32)
        ts = np.zeros(max(n_tag, 1), np.int32)
        info = CovInfo()
        _check(lib().arslam_lm_covariance(self._h, cap.ctypes.data_as(_dp), tag.ctypes.data_as(_dp), C.byref(var_f),
                                          cs.ctypes.data_as(_ip), ts.ctypes.data_as(_ip), C.byref(info)))
        return {"cap": cap, "tag": tag, "var_f": var_f.value, "cap_status": cs[:n_cap], "tag_status": ts[:n_tag],
                "info": info.to_dict()}

    def covariance_pairs(self, pairs):
        """Cross-covariance blocks at the point the last ``solve()`` returned
        (arslam_lm_covariance_pairs).  pairs: a sequence of ((kind_a, index_a), (kind_b, index_b)),
        kind BLOCK_CAMERA (index 0), BLOCK_CAPTURE or BLOCK_TAG.  Returns ``cov`` (n, 6, 6): rows
        of a by columns of b (a pair with the camera: cov(f, pose) in the first six values, var(f)
        at [0, 0] for the camera against itself, 0 elsewhere), ``status`` (n,) (COV_*) and ``info``."""
        flat = np.ascontiguousarray([[a[0], a[1], b[0], b[1]] for a, b in pairs], np.int32).reshape(-1, 4)
        n = len(flat)
        cov = np.zeros((n, 6, 6))
        st = np.zeros(max(n, 1), np.int32)
        info = CovInfo()
        _check(lib().arslam_lm_covariance_pairs(self._h, flat.ctypes.data_as(_ip) if n else None, C.c_int(n),
                                                cov.ctypes.data_as(_dp) if n else None, st.ctypes.data_as(_ip),
                                                C.byref(info)))
        return cov, st[:n], info.to_dict()

    def covariance_lens(self):
        """``covariance()`` with the camera block whole (arslam_lm_covariance_lens): ``cam`` (3, 3),
        the marginal of [f, l1, l2], and ``cam_status`` beside the other keys (``var_f`` = cam[0, 0]
        when the camera has a covariance, else -1).  Works under ``set_estimate_distortion``: l1, l2
        are then rows of H and every block is the marginal of that larger H.  Held l1, l2: their
        rows and columns of ``cam`` are 0 and the rest is ``covariance()``'s bits."""
        n_cap, n_tag = self.A.s.n_cap, self.A.s.n_tag
        cap = np.zeros((n_cap, 6, 6))
        tag = np.zeros((n_tag, 6, 6))
        cam = np.zeros((3, 3))
        cs = np.zeros(max(n_cap, 1), np.int32)
        ts = np.zeros(max(n_tag, 1), np.int32)
        cam_st = C.c_int(0)
        info = CovInfo()
        _check(lib().arslam_lm_covariance_lens(self._h, cap.ctypes.data_as(_dp), tag.ctypes.data_as(_dp),
                                               cam.ctypes.data_as(_dp), cs.ctypes.data_as(_ip),
                                               ts.ctypes.data_as(_ip), C.byref(cam_st), C.byref(info)))
        return {"cap": cap, "tag": tag, "cam": cam, "var_f": cam[0, 0] if cam_st.value == COV_OK else -1.0,
                "cap_status": cs[:n_cap], "tag_status": ts[:n_tag], "cam_status": cam_st.value,
                "info": info.to_dict()}

    def covariance_pairs_lens(self, pairs):
        """``covariance_pairs()`` over the matrix of ``covariance_lens()``
        (arslam_lm_covariance_pairs_lens): BLOCK_CAMERA is the 3-wide block [f, l1, l2] -- rows 0..2
        of the (6, 6) as a, columns 0..2 as b, the top-left (3, 3) against itself, 0 elsewhere."""
        flat = np.ascontiguousarray([[a[0], a[1], b[0], b[1]] for a, b in pairs], np.int32).reshape(-1, 4)
        n = len(flat)
        cov = np.zeros((n, 6, 6))
        st = np.zeros(max(n, 1), np.int32)
        info = CovInfo()
        _check(lib().arslam_lm_covariance_pairs_lens(self._h, flat.ctypes.data_as(_ip) if n else None, C.c_int(n),
                                                     cov.ctypes.data_as(_dp) if n else None, st.ctypes.data_as(_ip),
                                                     C.byref(info)))
        return cov, st[:n], info.to_dict()

    def debug_cov_camera_rows(self):
        """(rows (3, n_reduced + 1), row_slot (3,)): the camera's reduced rows f, l1, l2 of the
        covariance's reduced system at the point the last ``solve()`` returned -- no LM diagonal, the
        last column (the right-hand side) 0 (arslam_lm_debug_cov_camera_rows)."""
        cam = self.debug_reduced_rows()[2]
        n_cols = cam + 4
        rows = np.zeros((3, n_cols))
        slot = np.zeros(3, np.int32)
        _check(lib().arslam_lm_debug_cov_camera_rows(self._h, n_cols, rows.ctypes.data_as(_dp),
                                                     slot.ctypes.data_as(_ip)))
        return rows, slot

    def debug_reduced_rows(self):
        """(cap_row (n_cap,), tag_row (n_tag,), cam_row): the first reduced row of each block, -1 off
        the reduced side (arslam_lm_debug_reduced_rows)."""
        cr = np.zeros(max(self.A.s.n_cap, 1), np.int32)
        tr = np.zeros(max(self.A.s.n_tag, 1), np.int32)
        cam = C.c_int(-1)
        _check(lib().arslam_lm_debug_reduced_rows(self._h, cr.ctypes.data_as(_ip), tr.ctypes.data_as(_ip),
                                                  C.byref(cam)))
        return cr[:self.A.s.n_cap], tr[:self.A.s.n_tag], cam.value

    def debug_camera_rows(self, radius):
        """(rows (3, n_reduced + 1), row_slot (3,)): the camera's reduced rows f, l1, l2 of the
        assembled reduced system at the loaded point under the given radius, the last column the
        rows' right-hand side entries (arslam_lm_debug_camera_rows)."""
        cam = self.debug_reduced_rows()[2]
        n_cols = cam + 4
        rows = np.zeros((3, n_cols))
        slot = np.zeros(3, np.int32)
        _check(lib().arslam_lm_debug_camera_rows(self._h, float(radius), n_cols, rows.ctypes.data_as(_dp),
                                                 slot.ctypes.data_as(_ip)))
        return rows, slot

    def owned_captures(self):
        """Indices of the captures this rank owns (every capture on one rank)."""
        n = C.c_int(0)
        _check(lib().arslam_lm_owned_captures(self._h, None, C.c_int(0), C.byref(n)))
        out = (C.c_int * max(n.value, 1))()
        _check(lib().arslam_lm_owned_captures(self._h, out, C.c_int(n.value), C.byref(n)))
        return np.array(out[:n.value], np.int64)

    def debug_break_dependency(self, ticket):
        """Test hook: make one dependency wait of the factorization task graph unreachable."""
        out = C.c_long(-1)
        _check(lib().arslam_lm_debug_break_dependency(self._h, ticket, C.byref(out)))
        return out.value

    @property
    def camera(self):
        return self.A.camera

    @property
    def cap(self):
        return self.A.cap

    @property
    def tag(self):
        return self.A.tag


class Problem(_Handle):
    """ceres::Problem mirror with pointer-keyed parameter blocks (numpy arrays)."""

    def __init__(self, **opts):
        super().__init__(**opts)
        self._keep = []

    @staticmethod
    def _block(a, n):
        if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous
                and a.size == n):
            raise TypeError(f"parameter block must be a C-contiguous float64 array of size {n}")
        return a.ctypes.data_as(_dp)

    def add_residual_block(self, corners, camera, capture, tag, loss=None, size=None):
        """loss = (kind, a): this block's own robust loss; None: the handle's default (set_loss).
        size: the side of this block's tag in metres; None: the handle's default (set_tag_size)."""
        c = _f64(corners).reshape(8)
        self._keep += [camera, capture, tag]
        if size is not None:
            kind, a = self.get_loss() if loss is None else loss
            _check(lib().arslam_lm_add_residual_block_sized(self._h, c.ctypes.data_as(_dp),
                                                            self._block(camera, 3), self._block(capture, 6),
                                                            self._block(tag, 6), float(size), int(kind), float(a)))
            return
        if loss is not None:
            _check(lib().arslam_lm_add_residual_block_loss(self._h, c.ctypes.data_as(_dp),
                                                           self._block(camera, 3), self._block(capture, 6),
                                                           self._block(tag, 6), int(loss[0]), float(loss[1])))
            return
        _check(lib().arslam_lm_add_residual_block(self._h, c.ctypes.data_as(_dp),
                                                  self._block(camera, 3), self._block(capture, 6),
                                                  self._block(tag, 6)))

    def set_parameter_block_constant(self, block):
        _check(lib().arslam_lm_set_parameter_block_constant(self._h, block.ctypes.data_as(_dp)))

    def set_parameter_block_variable(self, block):
        _check(lib().arslam_lm_set_parameter_block_variable(self._h, block.ctypes.data_as(_dp)))

    def num_residual_blocks(self):
        return lib().arslam_lm_num_residual_blocks(self._h)

    def solve(self):
        s = Summary()
        _check(lib().arslam_lm_solve(self._h, C.byref(s)))
        return s.to_dict()

    def evaluate(self, apply_loss=True, residuals=True):
        """ceres::Problem::Evaluate over the residual blocks in the order they were added, at the
        values the blocks hold now (arslam_lm_evaluate_blocks): ``cost``, ``residuals`` (n, 8),
        ``sq_norm`` (n,), ``weight`` (n,) as ResidentProblem.evaluate; the gradient is kept on the
        handle for ``gradient_block``."""
        n = self.num_residual_blocks()
        out = _evaluate(lambda *a: lib().arslam_lm_evaluate_blocks(self._h, *a), 0, 0, n, apply_loss, residuals, None)
        del out["gradient"]
        return out

    def gradient_block(self, block):
        """The block's (3,) or (6,) entries of the gradient of the last ``evaluate()``
        (arslam_lm_gradient_block); an LMError (STATE) when the problem changed since."""
        if not (isinstance(block, np.ndarray) and block.dtype == np.float64 and block.size in (3, 6)):
            raise TypeError("parameter block must be a float64 array of size 3 or 6")
        out = np.zeros(block.size)
        _check(lib().arslam_lm_gradient_block(self._h, block.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
        return out

    def covariance_block(self, block):
        """Covariance::GetCovarianceBlock(block, block) after ``solve()``: (6, 6) for a pose block,
        (3, 3) for the camera block (var(f) at [0, 0]); and its status (COV_*)."""
        if not (isinstance(block, np.ndarray) and block.dtype == np.float64 and block.size in (3, 6)):
            raise TypeError("parameter block must be a float64 array of size 3 or 6")
        k = block.size
        out = np.zeros((k, k))
        st = C.c_int(0)
        _check(lib().arslam_lm_covariance_block(self._h, block.ctypes.data_as(_dp), out.ctypes.data_as(_dp),
                                                C.byref(st)))
        return out, st.value

    def covariance_block_pair(self, a, b):
        """Covariance::GetCovarianceBlock(a, b) after ``solve()`` in Ceres' shapes -- (6, 6), (3, 6),
        (6, 3) or (3, 3), the camera block 3 wide with cov(f, .) in its first row / column -- and its
        status (COV_*) (arslam_lm_covariance_block_pair)."""
        for blk in (a, b):
            if not (isinstance(blk, np.ndarray) and blk.dtype == np.float64 and blk.size in (3, 6)):
                raise TypeError("parameter block must be a float64 array of size 3 or 6")
        out = np.zeros((a.size, b.size))
        st = C.c_int(0)
        _check(lib().arslam_lm_covariance_block_pair(self._h, a.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                                     out.ctypes.data_as(_dp), C.byref(st)))
        return out, st.value

    def covariance_block_lens(self, block):
        """``covariance_block`` with the camera's (3, 3) over [f, l1, l2] whole
        (arslam_lm_covariance_block_lens); works under ``set_estimate_distortion``."""
        if not (isinstance(block, np.ndarray) and block.dtype == np.float64 and block.size in (3, 6)):
            raise TypeError("parameter block must be a float64 array of size 3 or 6")
        k = block.size
        out = np.zeros((k, k))
        st = C.c_int(0)
        _check(lib().arslam_lm_covariance_block_lens(self._h, block.ctypes.data_as(_dp), out.ctypes.data_as(_dp),
                                                     C.byref(st)))
        return out, st.value

    def covariance_block_pair_lens(self, a, b):
        """``covariance_block_pair`` with the camera block's three rows / columns [f, l1, l2]
        (arslam_lm_covariance_block_pair_lens); works under ``set_estimate_distortion``."""
        for blk in (a, b):
            if not (isinstance(blk, np.ndarray) and blk.dtype == np.float64 and blk.size in (3, 6)):
                raise TypeError("parameter block must be a float64 array of size 3 or 6")
        out = np.zeros((a.size, b.size))
        st = C.c_int(0)
        _check(lib().arslam_lm_covariance_block_pair_lens(self._h, a.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                                          out.ctypes.data_as(_dp), C.byref(st)))
        return out, st.value

    def reset(self):
        _check(lib().arslam_lm_reset(self._h))
        self._keep = []

    def debug_tag_pair_tile(self, tag_a, tag_b):
        """Where the loaded problem's reduced system couples tag blocks a and b: 2 an assembled
        tile, 1 a fill tile of the factor, 0 no tile, -1 not free tags (arslam_lm_debug.h)."""
        st = C.c_int(0)
        _check(lib().arslam_lm_debug_tag_pair_tile(self._h, self._block(tag_a, 6), self._block(tag_b, 6),
                                                   C.byref(st)))
        return st.value


# ---- component entry points (include/arslam_lm_debug.h) ----

def debug_slam_init_pose(which, rect, camera, pose_in, size=None):
    """The host mirror's initialisers alone (no device): which = "ar": initArPose from the capture's
    inv_pose, "capture": initCapturePose from the tag's pose; for a tag of side `size` (None: the
    call with the default argument).  arslam_slam_debug_init_pose."""
    rect, camera, pose_in = _f64(rect).reshape(8), _f64(camera).reshape(3), _f64(pose_in).reshape(6)
    out = np.zeros(6)
    _check(lib().arslam_slam_debug_init_pose({"ar": 0, "capture": 1}[which], rect.ctypes.data_as(_dp),
                                             camera.ctypes.data_as(_dp), pose_in.ctypes.data_as(_dp),
                                             0.0 if size is None else float(size), out.ctypes.data_as(_dp)))
    return out

def debug_residual_jacobian(cam, cap, tag, corners):
    """Device residuals (n,8) and Jacobians (n,8,15) of n independent observations."""
    cap = _f64(cap, (-1, 6))
    n = cap.shape[0]
    cam = _f64(np.broadcast_to(np.asarray(cam, np.float64), (n, 3)))
    tag = _f64(tag, (-1, 6))
    corners = _f64(corners, (-1, 8))
    r = np.zeros((n, 8))
    J = np.zeros((n, 8, 15))
    _check(lib().arslam_debug_residual_jacobian(n, cam.ctypes.data_as(_dp), cap.ctypes.data_as(_dp),
                                                tag.ctypes.data_as(_dp), corners.ctypes.data_as(_dp),
                                                r.ctypes.data_as(_dp), J.ctypes.data_as(_dp)))
    return r, J


def debug_residual_jacobian_sized(cam, cap, tag, corners, size):
    """debug_residual_jacobian for tags of side size[n] (metres; a scalar: every tag's)."""
    cap = _f64(cap, (-1, 6))
    n = cap.shape[0]
    cam = _f64(np.broadcast_to(np.asarray(cam, np.float64), (n, 3)))
    tag = _f64(tag, (-1, 6))
    corners = _f64(corners, (-1, 8))
    size = _f64(np.broadcast_to(np.asarray(size, np.float64), (n,)))
    r = np.zeros((n, 8))
    J = np.zeros((n, 8, 15))
    _check(lib().arslam_debug_residual_jacobian_sized(n, cam.ctypes.data_as(_dp), cap.ctypes.data_as(_dp),
                                                      tag.ctypes.data_as(_dp), corners.ctypes.data_as(_dp),
                                                      size.ctypes.data_as(_dp), r.ctypes.data_as(_dp),
                                                      J.ctypes.data_as(_dp)))
    return r, J


def debug_residual_jacobian_model(cam, cap, tag, corners, model, size=None):
    """debug_residual_jacobian under a camera model (CAMERA_*; cam rows = f, l1, l2), for tags of
    side size[n] (a scalar: every tag's; None: the default side)."""
    cap = _f64(cap, (-1, 6))
    n = cap.shape[0]
    cam = _f64(np.broadcast_to(np.asarray(cam, np.float64), (n, 3)))
    tag = _f64(tag, (-1, 6))
    corners = _f64(corners, (-1, 8))
    if size is not None:
        size = _f64(np.broadcast_to(np.asarray(size, np.float64), (n,)))
    r = np.zeros((n, 8))
    J = np.zeros((n, 8, 15))
    _check(lib().arslam_debug_residual_jacobian_model(n, int(model), cam.ctypes.data_as(_dp), cap.ctypes.data_as(_dp),
                                                      tag.ctypes.data_as(_dp), corners.ctypes.data_as(_dp),
                                                      size.ctypes.data_as(_dp) if size is not None else None,
                                                      r.ctypes.data_as(_dp), J.ctypes.data_as(_dp)))
    return r, J


def debug_residual_jacobian_distortion(cam, cap, tag, corners, size=None):
    """The radial model's residuals (n, 8) and the rows' two distortion columns (n, 8, 2),
    d r / d l1 and d r / d l2 (cam rows = f, l1, l2), for tags of side size[n] (None: default)."""
    cap = _f64(cap, (-1, 6))
    n = cap.shape[0]
    cam = _f64(np.broadcast_to(np.asarray(cam, np.float64), (n, 3)))
    tag = _f64(tag, (-1, 6))
    corners = _f64(corners, (-1, 8))
    if size is not None:
        size = _f64(np.broadcast_to(np.asarray(size, np.float64), (n,)))
    r = np.zeros((n, 8))
    Jl = np.zeros((n, 8, 2))
    _check(lib().arslam_debug_residual_jacobian_distortion(n, cam.ctypes.data_as(_dp), cap.ctypes.data_as(_dp),
                                                           tag.ctypes.data_as(_dp), corners.ctypes.data_as(_dp),
                                                           size.ctypes.data_as(_dp) if size is not None else None,
                                                           r.ctypes.data_as(_dp), Jl.ctypes.data_as(_dp)))
    return r, Jl


def debug_residual_jacobian_loss(cam, cap, tag, corners, kinds, a):
    """Device residuals (n,8) and Jacobians (n,8,15) of n independent observations after each one's
    robust loss (kinds[n] LOSS_*, a[n]): the rows times sqrt(rho'(s)); and rho(s) (n,)."""
    cap = _f64(cap, (-1, 6))
    n = cap.shape[0]
    cam = _f64(np.broadcast_to(np.asarray(cam, np.float64), (n, 3)))
    tag = _f64(tag, (-1, 6))
    corners = _f64(corners, (-1, 8))
    kinds = np.ascontiguousarray(np.broadcast_to(np.asarray(kinds), (n,)), np.uint8)
    a = _f64(np.broadcast_to(np.asarray(a, np.float64), (n,)))
    r = np.zeros((n, 8))
    J = np.zeros((n, 8, 15))
    rho = np.zeros(n)
    _check(lib().arslam_debug_residual_jacobian_loss(n, cam.ctypes.data_as(_dp), cap.ctypes.data_as(_dp),
                                                     tag.ctypes.data_as(_dp), corners.ctypes.data_as(_dp),
                                                     kinds.ctypes.data_as(_up), a.ctypes.data_as(_dp),
                                                     r.ctypes.data_as(_dp), J.ctypes.data_as(_dp),
                                                     rho.ctypes.data_as(_dp)))
    return r, J, rho


def debug_angle_axis_rotate(w, p):
    """Device AngleAxisRotatePoint of n points: (out (n,3), branch (n,) 1 = Rodrigues, 0 = small angle)."""
    w = _f64(w, (-1, 3))
    p = _f64(p, (-1, 3))
    n = w.shape[0]
    out = np.zeros((n, 3))
    br = np.zeros(n, np.int32)
    _check(lib().arslam_debug_angle_axis_rotate(n, w.ctypes.data_as(_dp), p.ctypes.data_as(_dp),
                                                out.ctypes.data_as(_dp), br.ctypes.data_as(_ip)))
    return out, br


def debug_dense_llt(A, b, executor=0):
    """Device Cholesky + solve of the SPD matrix A (lower triangle used). Returns (L, y, info)."""
    A = _f64(A).copy()
    n = A.shape[0]
    b = _f64(b).reshape(n)
    y = np.zeros(n)
    info = C.c_int(0)
    _check(lib().arslam_debug_dense_llt_ex(C.c_long(n), A.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                           y.ctypes.data_as(_dp), C.byref(info), C.c_int(executor)))
    return A, y, info.value


class TilePlanFacts(C.Structure):
    _fields_ = [("tiles_per_side", C.c_int), ("n_assembled", C.c_long), ("n_tiles", C.c_long),
                ("n_levels", C.c_int), ("n_split", C.c_long), ("n_dag_tasks", C.c_long),
                ("fill_first_ok", C.c_int), ("phase_split", C.c_long), ("grid", C.c_int * 2),
                ("n_cont_tasks", C.c_long), ("dag_valid", C.c_int)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["grid"] = tuple(self.grid)
        return d


def _u8_or_none(a, shape):
    return None if a is None else np.ascontiguousarray(np.asarray(a) != 0, np.uint8).reshape(shape)


def debug_tile_llt(A, b, tile_pattern=None, executor=0, col_class=None, fill_first=False):
    """Device Cholesky + solve of the SPD matrix A restricted to a lower tile pattern
    (arslam_debug_tile_llt): tile_pattern None (dense) or (T, T), T = (n + 1 + 63) // 64; col_class
    None or T values 0 / 1 (a two-phase plan on one rank); fill_first: the fill-first store over
    NaN fill tiles.  Returns (L (n, n), y, info, pattern (T, T) after fill, plan facts dict)."""
    A = _f64(A)
    n = A.shape[0]
    T = (n + 1 + 63) // 64
    b = _f64(b).reshape(n)
    pat = _u8_or_none(tile_pattern, (T, T))
    cls = _u8_or_none(col_class, (T,))
    Lf = np.zeros((n, n))
    y = np.zeros(n)
    out = np.zeros((T, T), np.uint8)
    info = C.c_int(0)
    facts = TilePlanFacts()
    _check(lib().arslam_debug_tile_llt(C.c_long(n), A.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                       pat.ctypes.data_as(_up) if pat is not None else None, C.c_int(executor),
                                       cls.ctypes.data_as(_up) if cls is not None else None,
                                       C.c_uint(1 if fill_first else 0), Lf.ctypes.data_as(_dp),
                                       y.ctypes.data_as(_dp), out.ctypes.data_as(_up), C.byref(info),
                                       C.byref(facts)))
    return Lf, y, info.value, out, facts.as_dict()


def debug_tile_plan(T, tile_pattern=None, col_class=None):
    """Host-only (no device): the plan debug_tile_llt builds for T tiles a side.  Returns (pattern
    (T, T) after fill, plan facts dict with dag_valid)."""
    pat = _u8_or_none(tile_pattern, (T, T))
    cls = _u8_or_none(col_class, (T,))
    out = np.zeros((T, T), np.uint8)
    facts = TilePlanFacts()
    _check(lib().arslam_debug_tile_plan(int(T), pat.ctypes.data_as(_up) if pat is not None else None,
                                        cls.ctypes.data_as(_up) if cls is not None else None,
                                        out.ctypes.data_as(_up), C.byref(facts)))
    return out, facts.as_dict()


def debug_selinv(A, tile_pattern=None):
    """Device selected inverse of the SPD matrix A on the tiles of its factor (the step behind
    ``covariance()``, alone).  tile_pattern: None for a dense matrix, else (T, T) with T =
    (n + 1 + 63) // 64, non-zero where lower tile (i, j) of A is taken.  Returns (Z (n, n): the
    inverse on the factor's tiles, 0 elsewhere; pattern (T, T): the factor's lower tile pattern; info)."""
    A = _f64(A)
    n = A.shape[0]
    T = (n + 1 + 63) // 64
    pat = None
    if tile_pattern is not None:
        pat = np.ascontiguousarray(tile_pattern, np.uint8).reshape(T, T)
    Z = np.zeros((n, n))
    out = np.zeros((T, T), np.uint8)
    info = C.c_int(0)
    _check(lib().arslam_debug_selinv(C.c_long(n), A.ctypes.data_as(_dp),
                                     pat.ctypes.data_as(_up) if pat is not None else None,
                                     Z.ctypes.data_as(_dp), out.ctypes.data_as(_up), C.byref(info)))
    return Z, out, info.value


def debug_tile_solve(A, B, tile_pattern=None):
    """X = A^-1 B from the device's multi-right-hand-side tile solve alone (the step behind
    ``covariance_pairs()``): A (n, n) SPD, factored as ``debug_selinv`` factors it, B (n, nrhs).
    Returns (X (n, nrhs), info)."""
    A = _f64(A)
    n = A.shape[0]
    B = np.ascontiguousarray(B, np.float64).reshape(n, -1)
    T = (n + 1 + 63) // 64
    pat = None
    if tile_pattern is not None:
        pat = np.ascontiguousarray(tile_pattern, np.uint8).reshape(T, T)
    X = np.zeros_like(B)
    info = C.c_int(0)
    _check(lib().arslam_debug_tile_solve(C.c_long(n), A.ctypes.data_as(_dp),
                                         pat.ctypes.data_as(_up) if pat is not None else None,
                                         C.c_int(B.shape[1]), B.ctypes.data_as(_dp), X.ctypes.data_as(_dp),
                                         C.byref(info)))
    return X, info.value


class PlanInfo(C.Structure):
    _fields_ = [("n_reduced", C.c_long), ("n_padded", C.c_long), ("pad_rows", C.c_long),
                ("tiles_per_side", C.c_int), ("n_parts", C.c_int), ("camera_row", C.c_int),
                ("n_levels", C.c_int), ("n_assembled_tiles", C.c_long), ("n_factor_tiles", C.c_long),
                ("n_update_tiles", C.c_long), ("n_update_items", C.c_long), ("n_split_targets", C.c_long),
                ("update_flops", C.c_double), ("n_dag_tasks", C.c_long), ("dag_valid", C.c_int),
                ("factor_flops", C.c_double), ("scalar_flops", C.c_double), ("fill_first_ok", C.c_int)]


def debug_reduced_plan(camera, cap, tag, obs_cap, obs_tag, corners, camera_const=False, cap_const=None,
                       tag_const=None, ordering=2, skip_zero_tiles=1):
    """Host-only symbolic analysis (no device): reduced layout + tile plan.  Returns (info dict, tag_row)."""
    A = _Soa(camera, cap, tag, obs_cap, obs_tag, corners, camera_const, cap_const, tag_const)
    info = PlanInfo()
    tag_row = np.zeros(max(A.tag.shape[0], 1), np.int32)
    _check(lib().arslam_debug_reduced_plan(C.byref(A.s), ordering, skip_zero_tiles, C.byref(info),
                                           tag_row.ctypes.data_as(_ip)))
    return {f: getattr(info, f) for f, _ in PlanInfo._fields_}, tag_row[:A.tag.shape[0]]


def debug_reduced_plan_side(camera, cap, tag, obs_cap, obs_tag, corners=None, elimination=ELIM_CAPTURES):
    """Host-only: the reduced layout and tile plan of a fresh one-rank load under elimination
    (ELIM_CAPTURES, ELIM_TAGS or ELIM_MIXED).  Returns (side used, info dict)."""
    if corners is None:
        corners = np.zeros((len(obs_cap), 8))
    A = _Soa(camera, cap, tag, obs_cap, obs_tag, corners, False, None, None)
    info = PlanInfo()
    side = lib().arslam_debug_reduced_plan_side(C.byref(A.s), elimination, C.byref(info))
    _check(min(side, 0))
    return side, {f: getattr(info, f) for f, _ in PlanInfo._fields_}


class OrderStep(C.Structure):
    _fields_ = [("side", C.c_int), ("order_reused", C.c_int), ("recomputed", C.c_int), ("etree_height", C.c_int),
                ("pad_rows", C.c_long)]


def debug_order_memory(problems, elimination=ELIM_CAPTURES, ordering=2, forget_before=None):
    """Host-only: the problems in turn through one elimination-order memory, the first as a first
    one-rank load, each later one as a pointer-keyed reload that may keep the remembered order
    (forget_before[i]: drop the memory before problem i, as a reset does).  problems: dicts with
    camera, cap, tag, obs_cap, obs_tag and optionally corners, camera_const, cap_const, tag_const.
    Returns one dict per problem: side, order_reused, recomputed (a kept order replaced because its
    tile elimination tree grew too tall), etree_height, pad_rows, and tag_row / cap_row: the first
    reduced row of each original tag / capture, -1 for none."""
    soas = [_Soa(q["camera"], q["cap"], q["tag"], q["obs_cap"], q["obs_tag"],
                 q["corners"] if q.get("corners") is not None else np.zeros((len(q["obs_cap"]), 8)),
                 q.get("camera_const", False), q.get("cap_const"), q.get("tag_const")) for q in problems]
    n = len(soas)
    arr = (SoaProblem * n)(*[A.s for A in soas])
    steps = (OrderStep * n)()
    tag_rows = [np.zeros(max(A.tag.shape[0], 1), np.int32) for A in soas]
    cap_rows = [np.zeros(max(A.cap.shape[0], 1), np.int32) for A in soas]
    tr = (_ip * n)(*[r.ctypes.data_as(_ip) for r in tag_rows])
    cr = (_ip * n)(*[r.ctypes.data_as(_ip) for r in cap_rows])
    fb = None
    if forget_before is not None:
        fb = np.ascontiguousarray(forget_before, np.uint8)
        assert fb.shape == (n,)
    L = lib()
    L.arslam_debug_order_memory.argtypes = [C.POINTER(SoaProblem), C.c_int, C.c_int, C.c_int, _up,
                                            C.POINTER(OrderStep), C.POINTER(_ip), C.POINTER(_ip)]
    _check(L.arslam_debug_order_memory(arr, n, int(elimination), int(ordering),
                                       fb.ctypes.data_as(_up) if fb is not None else None, steps, tr, cr))
    out = []
    for i, A in enumerate(soas):
        d = {f: getattr(steps[i], f) for f, _ in OrderStep._fields_}
        d["tag_row"] = tag_rows[i][:A.tag.shape[0]]
        d["cap_row"] = cap_rows[i][:A.cap.shape[0]]
        out.append(d)
    return out


def box_fingerprint(device=0):
    """The device's hand-off round trips (arslam_debug_box_fingerprint), a few ms of GPU time:
    the kind of MI355X box a measurement ran on."""
    out = (C.c_double * 6)()
    _check(lib().arslam_debug_box_fingerprint(int(device), out))
    return {"cas_poll_ns": out[0], "sc1_load_ns": out[1], "wt_store_ack_ns": out[2],
            "pingpong_ns": out[3], "pingpong_xcc": [int(out[4]), int(out[5])]}


def debug_dag_simulate(g, n_workers, seed=1, policy=0, started=None):
    """Host-only: one simulated interleaving of the persistent executor's protocol on g's one-rank
    plan (policy 0 random, 1-3 adversarial; + 16 without the in-flight cap on claimed targets;
    + 32 with round 5's cap, half the grid).  started=k: only k of the n_workers workgroups ever
    start.  True if every task finished, False on a deadlock."""
    A = _Soa(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    ok = C.c_int(-1)
    if started is None:
        _check(lib().arslam_debug_dag_simulate(C.byref(A.s), int(n_workers), C.c_uint(seed), int(policy),
                                               C.byref(ok)))
    else:
        _check(lib().arslam_debug_dag_simulate_started(C.byref(A.s), int(n_workers), int(started), C.c_uint(seed),
                                                       int(policy), C.byref(ok)))
    return bool(ok.value)


def debug_dag_workgroup_limit(k):
    """Process-wide test knob: later k_factor_dag launches let only their first k workgroups start
    (as if only k were resident); k <= 0 restores the whole grid."""
    _check(lib().arslam_debug_dag_workgroup_limit(int(k)))


def debug_dag_fault_detail(g, rec):
    """Host-only: the text an executor fault carries for fault record rec[8] (llt_plan.h
    DagFaultField) on g's one-rank plan."""
    A = _Soa(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    r = (C.c_int * 9)(*([int(v) for v in rec] + [0] * (9 - len(rec))))
    buf = C.create_string_buffer(4096)
    _check(lib().arslam_debug_dag_fault_detail(C.byref(A.s), r, buf, len(buf)))
    return buf.value.decode()


def debug_gather_extend(camera, cap, tag, obs_cap, obs_tag, corners, c0):
    """Host-only: the appended-problem Schur gather plan (the first c0 captures' plan extended by the
    rest) against a fresh plan of the whole problem.  Returns (identical, n_destinations)."""
    A = _Soa(camera, cap, tag, obs_cap, obs_tag, corners)
    same, nd = C.c_int(0), C.c_int(0)
    _check(lib().arslam_debug_gather_extend(C.byref(A.s), c0, C.byref(same), C.byref(nd)))
    return bool(same.value), nd.value


def debug_schur_store_table(nblk):
    """Host-only: k_schur's output-stage descriptors for captures of nblk distinct tags (1..10), in
    kernel order [tile (r, cc), cc <= r + 1][lane][register]: (offset, stored) -- the element's offset
    in the capture's block-packed slab and whether the lane stores it."""
    off = np.zeros((13, 64, 4), np.int32)
    stored = np.zeros((13, 64, 4), np.uint8)
    _check(lib().arslam_debug_schur_store_table(int(nblk), off.ctypes.data_as(_ip),
                                                stored.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return off, stored


class SplitInfo(C.Structure):
    _fields_ = [("tiles_per_side", C.c_int), ("n_top_cols", C.c_int), ("n_own_cols", C.c_int),
                ("n_top_tiles", C.c_long), ("n_tiles", C.c_long), ("n_dag_tasks", C.c_long),
                ("phase_split", C.c_long), ("dag_valid", C.c_int), ("n_owned_captures", C.c_int),
                ("top_work", C.c_double), ("max_rank_work", C.c_double), ("total_work", C.c_double),
                ("n_active", C.c_int)]


def debug_rank_split(camera, cap, tag, obs_cap, obs_tag, corners, nranks, rank):
    """Host-only: the multi-rank split the solver makes for `rank` of `nranks` (two-phase tile
    plan of that rank, its validity) and every capture's owner.  Returns (info dict, cap_owner)."""
    A = _Soa(camera, cap, tag, obs_cap, obs_tag, corners)
    info = SplitInfo()
    owner = np.zeros(max(A.cap.shape[0], 1), np.int32)
    _check(lib().arslam_debug_rank_split(C.byref(A.s), nranks, rank, C.byref(info), owner.ctypes.data_as(_ip)))
    return {f: getattr(info, f) for f, _ in SplitInfo._fields_}, owner[:A.cap.shape[0]]


def debug_dag_tasks(g, nranks=1, rank=0):
    """Host-only: the factorization's task graph in the plan the solver makes for `rank` of `nranks`
    (1: the one-rank plan).  Returns {"tasks": [n, 4] (type, y, z, w; type 0 POTRF k = y, 1 TRSM,
    2 update item, 3 INV k = y) in ticket order, "phase": [n], "T", "phase_split", "n_phases",
    "root_inv_col": the column whose POTRF task also inverts L_kk and that has no INV task, or -1}."""
    A = _Soa(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    n, info = C.c_long(0), (C.c_int * 4)()
    _check(lib().arslam_debug_dag_tasks(C.byref(A.s), int(nranks), int(rank), None, None, 0, C.byref(n), info))
    tasks, phase = np.zeros((max(n.value, 1), 4), np.int32), np.zeros(max(n.value, 1), np.int32)
    _check(lib().arslam_debug_dag_tasks(C.byref(A.s), int(nranks), int(rank), tasks.ctypes.data_as(_ip),
                                        phase.ctypes.data_as(_ip), n.value, C.byref(n), info))
    return {"tasks": tasks[:n.value], "phase": phase[:n.value], "T": info[0], "phase_split": info[1],
            "n_phases": info[2], "root_inv_col": info[3]}


def debug_ceres_e_blocks(camera, cap, tag, obs_cap, obs_tag, corners=None, camera_const=False, cap_const=None,
                         tag_const=None):
    """Host-only: Ceres 2.0's DENSE_SCHUR e-block set (the rule ELIM_AUTO follows), as
    {captures, tags, camera, max_tag_obs}."""
    if corners is None:
        corners = np.zeros((len(obs_cap), 8))
    A = _Soa(camera, cap, tag, obs_cap, obs_tag, corners, camera_const, cap_const, tag_const)
    out = np.zeros(4, np.int32)
    _check(lib().arslam_debug_ceres_e_blocks(C.byref(A.s), out.ctypes.data_as(_ip)))
    return dict(captures=int(out[0]), tags=int(out[1]), camera=int(out[2]), max_tag_obs=int(out[3]))


def debug_mixed_groups(camera, cap, tag, obs_cap, obs_tag, corners=None, camera_const=False, cap_const=None,
                       tag_const=None):
    """Host-only: Ceres' e-block set (e_cap, e_tag: 0/1 per capture / tag) and the ELIM_MIXED
    device problem's {groups, f_blocks, direct, max_blk}."""
    if corners is None:
        corners = np.zeros((len(obs_cap), 8))
    A = _Soa(camera, cap, tag, obs_cap, obs_tag, corners, camera_const, cap_const, tag_const)
    out = np.zeros(4, np.int32)
    e_cap = np.zeros(max(A.cap.shape[0], 1), np.uint8)
    e_tag = np.zeros(max(A.tag.shape[0], 1), np.uint8)
    _check(lib().arslam_debug_mixed_groups(C.byref(A.s), out.ctypes.data_as(_ip),
                                           e_cap.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                           e_tag.ctypes.data_as(C.POINTER(C.c_ubyte))))
    return dict(groups=int(out[0]), f_blocks=int(out[1]), direct=int(out[2]), max_blk=int(out[3]),
                e_cap=e_cap[:A.cap.shape[0]], e_tag=e_tag[:A.tag.shape[0]])


# ---- batched localize (include/arslam_localize.h) ----
LOC_SKIPPED = -1
COV_OK, COV_UNAVAILABLE, COV_RANK_DEFICIENT = 0, 1, 2   # arslam_localize.h ARSLAM_COV_*


class LocalizeBatchC(C.Structure):
    _fields_ = [("n_query", C.c_int), ("n_tag", C.c_int), ("n_obs", C.c_int),
                ("camera", _dp), ("tag", _dp), ("tag_in_map", _up), ("query_start", _ip),
                ("obs_tag", _ip), ("corners", _dp), ("pose", _dp), ("init_from_map", C.c_int)]


class LocalizeResult(C.Structure):
    _fields_ = [("status", C.c_int), ("rule", C.c_int), ("num_iterations", C.c_int),
                ("num_successful_steps", C.c_int), ("num_unsuccessful_steps", C.c_int),
                ("init_obs", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double)]


def _loc_results(res):
    n = len(res)
    f = {k: np.array([getattr(r, k) for r in res]) for k, _ in LocalizeResult._fields_}
    f["rule_name"] = [RULES.get(r, str(r)) for r in f["rule"]] if n else []
    return f


class _LocArrays:
    def __init__(self, batch, init_from_map, pose):
        self.camera = _f64(batch.camera).copy()
        self.tag = _f64(batch.tag, (-1, 6)).copy()
        self.q_start = np.ascontiguousarray(batch.q_start, np.int32)
        self.obs_tag = np.ascontiguousarray(batch.obs_tag, np.int32)
        self.corners = _f64(batch.corners, (-1, 8))
        nq = self.q_start.shape[0] - 1
        self.pose = np.zeros((nq, 6)) if pose is None else _f64(pose, (-1, 6)).copy()
        tim = getattr(batch, "tag_in_map", None)
        self.tim = None if tim is None else np.ascontiguousarray(tim, np.uint8)
        self.s = LocalizeBatchC(nq, self.tag.shape[0], self.obs_tag.shape[0],
                                self.camera.ctypes.data_as(_dp), self.tag.ctypes.data_as(_dp),
                                None if self.tim is None else self.tim.ctypes.data_as(_up),
                                self.q_start.ctypes.data_as(_ip), self.obs_tag.ctypes.data_as(_ip),
                                self.corners.ctypes.data_as(_dp), self.pose.ctypes.data_as(_dp),
                                int(bool(init_from_map)))


def localize_many(batch, init_from_map=True, pose=None, loss=None, covariance=False, tag_size=None, **opts):
    """localizeMany on the device (one-shot).  ``batch`` has camera, tag, q_start, obs_tag,
    corners, tag_in_map (synth.LocalizeBatch).  loss = (kind, a): every observation's robust loss
    (LOSS_*, scale); the results' costs are then the robust cost.  tag_size: the map tags' sides in
    metres, [n_tag] or a scalar (None: DEFAULT_TAG_SIZE).  Returns (pose (Nq,6), results
    dict of arrays); with covariance=True also cov (Nq, 6, 6) and its status (Nq,), COV_*
    (Localizer.covariance)."""
    A = _LocArrays(batch, init_from_map, pose)
    res = (LocalizeResult * max(A.s.n_query, 1))()
    if tag_size is not None:
        nq = A.s.n_query
        sizes = _f64(np.broadcast_to(np.asarray(tag_size, np.float64), (A.s.n_tag,)))
        cov, st = np.zeros((max(nq, 1), 6, 6)), np.zeros(max(nq, 1), np.int32)
        kind, a = (LOSS_NONE, 0.0) if loss is None else loss
        _check(lib().arslam_localize_many_sized(C.byref(A.s), C.byref(make_options(**opts)), sizes.ctypes.data_as(_dp),
                                                int(kind), float(a), res,
                                                cov.ctypes.data_as(_dp) if covariance else None,
                                                st.ctypes.data_as(_ip) if covariance else None))
        out = (A.pose, _loc_results(res[:nq]))
        return out + (cov[:nq], st[:nq]) if covariance else out
    if covariance:
        nq = A.s.n_query
        cov, st = np.zeros((max(nq, 1), 6, 6)), np.zeros(max(nq, 1), np.int32)
        kind, a = (LOSS_NONE, 0.0) if loss is None else loss
        _check(lib().arslam_localize_many_cov(C.byref(A.s), C.byref(make_options(**opts)), int(kind), float(a), res,
                                              cov.ctypes.data_as(_dp), st.ctypes.data_as(_ip)))
        return A.pose, _loc_results(res[:nq]), cov[:nq], st[:nq]
    if loss is None:
        _check(lib().arslam_localize_many(C.byref(A.s), C.byref(make_options(**opts)), res))
    else:
        _check(lib().arslam_localize_many_loss(C.byref(A.s), C.byref(make_options(**opts)), int(loss[0]),
                                               float(loss[1]), res))
    return A.pose, _loc_results(res[:A.s.n_query])


class Localizer:
    """Resident batched localizer: load a batch once, solve it many times."""

    def __init__(self, batch, init_from_map=True, pose=None, loss=None, obs_loss=None, tag_size=None,
                 camera_model=None, **opts):
        """loss = (kind, a): the robust loss of every observation (the handle's default loss);
        obs_loss = (kinds[n_obs], a[n_obs]): one loss per observation of this batch, in observation
        order, overriding the default; tag_size: the map tags' sides in metres, [n_tag] or a scalar
        (None: DEFAULT_TAG_SIZE); camera_model = CAMERA_PINHOLE / CAMERA_RADIAL (None: PINHOLE)."""
        self._h = C.c_void_p()
        _check(lib().arslam_localizer_create(C.byref(self._h), C.byref(make_options(**opts))))
        if camera_model is not None:
            self.set_camera_model(camera_model)
        self.A = _LocArrays(batch, init_from_map, pose)
        self.n_query = self.A.s.n_query
        self.n_obs = self.A.s.n_obs
        if loss is not None:
            self.set_loss(*loss)
        kinds = scales = None
        if obs_loss is not None:
            kinds = np.ascontiguousarray(obs_loss[0], np.uint8).reshape(-1)
            scales = _f64(obs_loss[1]).reshape(-1)
            if kinds.shape[0] != self.n_obs or scales.shape[0] != self.n_obs:
                raise ValueError("obs_loss: one kind and one scale per observation")
        if tag_size is not None:
            sizes = _f64(np.broadcast_to(np.asarray(tag_size, np.float64), (self.A.s.n_tag,)))
            _check(lib().arslam_localizer_load_sized(self._h, C.byref(self.A.s), sizes.ctypes.data_as(_dp),
                                                     kinds.ctypes.data_as(_up) if kinds is not None else None,
                                                     scales.ctypes.data_as(_dp) if scales is not None else None))
        elif obs_loss is None:
            _check(lib().arslam_localizer_load(self._h, C.byref(self.A.s)))
        else:
            _check(lib().arslam_localizer_load_loss(self._h, C.byref(self.A.s), kinds.ctypes.data_as(_up),
                                                    scales.ctypes.data_as(_dp)))

    def set_camera_model(self, model):
        """CAMERA_PINHOLE or CAMERA_RADIAL (l1, l2 = the batch's camera[1], camera[2]): the model
        of solve(), observation_terms() and covariance(); the batch stays loaded."""
        _check(lib().arslam_localizer_set_camera_model(self._h, int(model)))

    def camera_model(self):
        m = C.c_int(0)
        _check(lib().arslam_localizer_camera_model(self._h, C.byref(m)))
        return m.value

    def set_tag_size(self, size):
        """The default side (metres) of every map tag of a batch loaded afterwards."""
        _check(lib().arslam_localizer_set_tag_size(self._h, float(size)))

    def get_tag_size(self):
        s = C.c_double(0.0)
        _check(lib().arslam_localizer_get_tag_size(self._h, C.byref(s)))
        return s.value

    def set_loss(self, kind, a=0.0):
        """The default loss (LOSS_*, scale a) of every observation, from the next solve() on; the
        loaded batch stays loaded.  A batch loaded with obs_loss keeps its own losses."""
        _check(lib().arslam_localizer_set_loss(self._h, int(kind), float(a)))

    def get_loss(self):
        """(kind, a) of the default loss."""
        k, a = C.c_int(0), C.c_double(0.0)
        _check(lib().arslam_localizer_get_loss(self._h, C.byref(k), C.byref(a)))
        return k.value, a.value

    def observation_terms(self):
        """(s, w), each (n_obs,): per observation the plain squared residual s = |r|^2 and the
        weight w = rho'(s) at the poses the last solve() returned (w = 1 without a loss, near 0 for
        a rejected detection); -1 for the observations of skipped queries."""
        s, w = np.zeros(max(self.n_obs, 1)), np.zeros(max(self.n_obs, 1))
        _check(lib().arslam_localizer_observation_terms(self._h, s.ctypes.data_as(_dp), w.ctypes.data_as(_dp)))
        return s[:self.n_obs], w[:self.n_obs]

    def covariance(self, timed=False):
        """(cov (n_query, 6, 6), status (n_query,), min_pivot (n_query,)): per query the inverse
        of J~'J~ at the pose the last solve() returned, rows corrected by the loss as in the solve
        (ceres::Covariance with apply_loss_function), parameters [t_c, w_c], for unit-variance
        residuals (multiply by the pixel noise's sigma^2); status COV_OK, COV_UNAVAILABLE (skipped
        or failed evaluation) or COV_RANK_DEFICIENT, the last two with cov = -1; min_pivot the
        smallest squared pivot of the equilibrated Cholesky.  timed=True appends the kernel's
        device time in ms."""
        nq = self.n_query
        cov, st, mp = np.zeros((max(nq, 1), 6, 6)), np.zeros(max(nq, 1), np.int32), np.zeros(max(nq, 1))
        ms = C.c_double(0.0)
        args = (self._h, cov.ctypes.data_as(_dp), st.ctypes.data_as(_ip), mp.ctypes.data_as(_dp))
        if timed:
            _check(lib().arslam_localizer_covariance_timed(*args, C.byref(ms)))
            return cov[:nq], st[:nq], mp[:nq], ms.value
        _check(lib().arslam_localizer_covariance(*args))
        return cov[:nq], st[:nq], mp[:nq]

    def solve(self, download=True):
        """Returns (pose or None, results or None, kernel_ms)."""
        ms = C.c_double(0.0)
        pose = np.zeros((self.n_query, 6)) if download else None
        res = (LocalizeResult * max(self.n_query, 1))() if download else None
        _check(lib().arslam_localizer_solve(self._h, None if pose is None else pose.ctypes.data_as(_dp),
                                            res, C.byref(ms)))
        return pose, (None if res is None else _loc_results(res[:self.n_query])), ms.value

    def close(self):
        if self._h:
            lib().arslam_localizer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- ArSlamSolver host mirror (include/arslam_slam.h) ----
class Transform(C.Structure):
    _fields_ = [("child_frame_id", C.c_char * 128), ("translation", C.c_double * 3),
                ("rotation", C.c_double * 4)]


class SlamSolver:
    """ArSlamSolver (ar_slam_util.hpp:361-497) over the C++ host mirror: captures, arucos and
    blocks addressed by index; uids / ids are strings."""

    def __init__(self, verbose=False, **opts):
        self._h = C.c_void_p()
        _check(lib().arslam_slam_create(C.byref(self._h), C.byref(make_options(**opts))))
        lib().arslam_slam_set_verbose(self._h, int(bool(verbose)))

    def close(self):
        if self._h:
            lib().arslam_slam_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_loss(self, kind, a=0.0):
        """The robust loss (LOSS_*, scale a) of every residual block added from now on: solve,
        solve_incremental and the solveCapture calls inside them.  localize_many has its own:
        set_localize_loss."""
        _check(lib().arslam_slam_set_loss(self._h, int(kind), C.c_double(float(a))))

    def set_localize_loss(self, kind, a=0.0):
        """The robust loss (LOSS_*, scale a) of every residual block localize_many adds."""
        _check(lib().arslam_slam_set_localize_loss(self._h, int(kind), C.c_double(float(a))))

    def set_default_aruco_size(self, size):
        """The side (metres) of the tags created from now on (DEFAULT_TAG_SIZE initially)."""
        _check(lib().arslam_slam_set_default_aruco_size(self._h, float(size)))

    def set_aruco_size(self, tag_id, size):
        """The side (metres) of the tag with this id string; may precede its first detection.
        STATE once the tag is initialised or has residual blocks."""
        _check(lib().arslam_slam_set_aruco_size(self._h, str(tag_id).encode(), float(size)))

    def aruco_size(self, a):
        s = C.c_double(0.0)
        _check(lib().arslam_slam_aruco_size(self._h, int(a), C.byref(s)))
        return s.value

    def set_camera_model(self, model):
        """CAMERA_PINHOLE or CAMERA_RADIAL for the mapper and the localizer the solver keeps.
        STATE once residual blocks have been added."""
        _check(lib().arslam_slam_set_camera_model(self._h, int(model)))

    def camera_model(self):
        m = C.c_int(0)
        _check(lib().arslam_slam_camera_model(self._h, C.byref(m)))
        return m.value

    def camera_distortion(self):
        """The plumb_bob vector beside camera_info: [l1, l2, 0, 0, 0] under RADIAL, else zeros."""
        d = np.zeros(5)
        _check(lib().arslam_slam_camera_distortion(self._h, d.ctypes.data_as(_dp)))
        return d

    def load_yaml(self, path):
        _check(lib().arslam_slam_load_yaml(self._h, str(path).encode()))

    def load_yaml_string(self, text):
        _check(lib().arslam_slam_load_yaml_string(self._h, text.encode()))

    def save_yaml(self, path):
        _check(lib().arslam_slam_save_yaml(self._h, str(path).encode()))

    def add_detections(self, capture_uid, ids, corners, image_width=1020, image_height=768, image_path=""):
        """Detections.msg -> capture index, or None when ignored (addDetections :591-627)."""
        corners = _f64(corners, (-1, 8))
        n = corners.shape[0]
        if len(ids) != n:
            raise ValueError("one id per detection")
        arr = (C.c_char_p * max(n, 1))(*[str(i).encode() for i in ids])
        idx = C.c_int(-1)
        _check(lib().arslam_slam_add_detections(self._h, str(capture_uid).encode(), C.c_int(image_width),
                                                C.c_int(image_height), str(image_path).encode(), C.c_int(n),
                                                arr, corners.ctypes.data_as(_dp), C.byref(idx)))
        return None if idx.value < 0 else idx.value

    def solve(self):
        _check(lib().arslam_slam_solve(self._h))

    def solve_incremental(self):
        _check(lib().arslam_slam_solve_incremental(self._h))

    def localize_many(self, first_loc_cap_idx):
        _check(lib().arslam_slam_localize_many(self._h, C.c_int(first_loc_cap_idx)))

    def localize_covariance(self, cap_idx):
        """(cov (6, 6), status COV_*) of a capture the last localize_many localized
        (Localizer.covariance); LMError -7 (STATE) for any other capture."""
        cov, st = np.zeros((6, 6)), C.c_int(-1)
        _check(lib().arslam_slam_localize_covariance(self._h, int(cap_idx), cov.ctypes.data_as(_dp), C.byref(st)))
        return cov, st.value

    def evaluate(self):
        """ceres::Problem::Evaluate on the mapper problem at the current poses
        (arslam_slam_evaluate): {cost, sq_norm (num_blocks,), weight (num_blocks,)}, the block's
        |r|^2 and loss weight rho' under the loss it was added with; -1 in both for a block that
        is not in the problem."""
        n = lib().arslam_slam_num_blocks(self._h)
        cost = C.c_double(0.0)
        sq, w = np.zeros(max(n, 1)), np.zeros(max(n, 1))
        _check(lib().arslam_slam_evaluate(self._h, C.byref(cost), sq.ctypes.data_as(_dp), w.ctypes.data_as(_dp)))
        return {"cost": cost.value, "sq_norm": sq[:n], "weight": w[:n]}

    @property
    def num_captures(self):
        return lib().arslam_slam_num_captures(self._h)

    @property
    def num_arucos(self):
        return lib().arslam_slam_num_arucos(self._h)

    @property
    def num_blocks(self):
        return lib().arslam_slam_num_blocks(self._h)

    @property
    def num_solves(self):
        return lib().arslam_slam_num_solves(self._h)

    def last_summary(self):
        s = Summary()
        _check(lib().arslam_slam_last_summary(self._h, C.byref(s)))
        return s.to_dict()

    def solve_summary(self, i):
        """Summary of optimize() call i."""
        s = Summary()
        _check(lib().arslam_slam_solve_summary(self._h, C.c_int(i), C.byref(s)))
        return s.to_dict()

    def solve_capture(self, i):
        """Index of the capture whose optimize() was call i (the drivers' visiting order)."""
        c = C.c_int(-1)
        _check(lib().arslam_slam_solve_capture(self._h, C.c_int(i), C.byref(c)))
        return c.value

    def solve_order(self):
        return [self.solve_capture(i) for i in range(self.num_solves)]

    def unsolved_captures(self):
        """The unsolved-capture set in its iteration order (begin() first)."""
        n = C.c_int(0)
        _check(lib().arslam_slam_unsolved_captures(self._h, None, C.c_int(0), C.byref(n)))
        out = (C.c_int * max(n.value, 1))()
        _check(lib().arslam_slam_unsolved_captures(self._h, out, C.c_int(n.value), C.byref(n)))
        return [int(out[i]) for i in range(n.value)]

    def capture(self, c):
        buf = C.create_string_buffer(256)
        pose = np.zeros(6)
        _check(lib().arslam_slam_capture(self._h, C.c_int(c), buf, C.c_int(256), pose.ctypes.data_as(_dp)))
        return buf.value.decode(), pose

    def set_capture_pose(self, c, pose):
        p = _f64(pose).reshape(6).copy()
        _check(lib().arslam_slam_set_capture_pose(self._h, C.c_int(c), p.ctypes.data_as(_dp)))

    def aruco(self, a):
        buf = C.create_string_buffer(256)
        pose = np.zeros(6)
        init = C.c_int(0)
        _check(lib().arslam_slam_aruco(self._h, C.c_int(a), buf, C.c_int(256), pose.ctypes.data_as(_dp),
                                       C.byref(init)))
        return buf.value.decode(), pose, bool(init.value)

    def set_aruco_pose(self, a, pose):
        p = _f64(pose).reshape(6).copy()
        _check(lib().arslam_slam_set_aruco_pose(self._h, C.c_int(a), p.ctypes.data_as(_dp)))

    def block(self, b):
        c, a, added = C.c_int(), C.c_int(), C.c_int()
        rect = np.zeros(8)
        _check(lib().arslam_slam_block(self._h, C.c_int(b), C.byref(c), C.byref(a), rect.ctypes.data_as(_dp),
                                       C.byref(added)))
        return c.value, a.value, rect, bool(added.value)

    def camera(self):
        p = np.zeros(3)
        w, h = C.c_int(), C.c_int()
        _check(lib().arslam_slam_camera(self._h, p.ctypes.data_as(_dp), C.byref(w), C.byref(h)))
        return p, (None if w.value < 0 else (w.value, h.value))

    def set_camera(self, params):
        p = _f64(params).reshape(3).copy()
        _check(lib().arslam_slam_set_camera(self._h, p.ctypes.data_as(_dp)))

    def capture_poses(self):
        return np.array([self.capture(c)[1] for c in range(self.num_captures)]).reshape(-1, 6)

    def aruco_poses(self):
        return np.array([self.aruco(a)[1] for a in range(self.num_arucos)]).reshape(-1, 6)

    def get_transforms(self):
        n = C.c_int(0)
        _check(lib().arslam_slam_get_transforms(self._h, None, C.c_int(0), C.byref(n)))
        arr = (Transform * max(n.value, 1))()
        _check(lib().arslam_slam_get_transforms(self._h, arr, C.c_int(n.value), C.byref(n)))
        return [(t.child_frame_id.decode(), np.array(t.translation[:]), np.array(t.rotation[:]))
                for t in arr[:n.value]]

    def camera_info(self):
        k, p = np.zeros(9), np.zeros(12)
        _check(lib().arslam_slam_camera_info(self._h, k.ctypes.data_as(_dp), p.ctypes.data_as(_dp)))
        return k.reshape(3, 3), p.reshape(3, 4)
