"""Python binding of libarslam_lm.so (ctypes over the C-ABI in include/*.h).

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

One module per header: ``mapper`` (arslam_lm.h), ``localize`` (arslam_localize.h), ``slam``
(arslam_slam.h) and ``debug`` (arslam_lm_debug.h), over ``_abi``: the struct mirrors, the table
of every symbol's signature and the loaded library.  Everything is used as ``lm.X``.

There is no CPU fallback: if the HIP library is missing or no GPU is
present, construction raises.
"""
from ._abi import *   # noqa: F401,F403 -- the constants, the struct mirrors, lib() and its helpers
from ._abi import _check, _dp, _ip, _up   # noqa: F401 -- (the tests call the ABI directly with these)
from .debug import *   # noqa: F401,F403
from .localize import Localizer, _LocArrays, localize_many   # noqa: F401
from .mapper import (Problem, ResidentProblem, _Handle, _Soa, comm_unique_id, solve_graph, solve_soa,   # noqa: F401
                     warm_up)
from .slam import SlamSolver   # noqa: F401
