"""Return codes of the component entry points (include/arslam_lm_debug.h), called through raw
ctypes: every argument check that answers before any device call, and what the device entry
points answer on a host without a GPU (CPU only)."""
import ctypes as C

import numpy as np
import pytest

from ar_slam_amd import synth

OK, E_INVALID_ARG, E_HIP = 0, -1, -4


@pytest.fixture(scope="module")
def L():
    from ar_slam_amd import build, lm
    build.build()
    return lm


@pytest.fixture(scope="module")
def soa(L):
    g = synth.config_graph("small")
    return L._Soa(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _up(a):
    return None if a is None else np.ascontiguousarray(a, np.uint8).ctypes.data_as(C.POINTER(C.c_ubyte))


def _tile_llt(L, n, executor=0, flags=0, col_class=None, null_A=False, m=None):
    m = max(n, 1) if m is None else m
    A, b, Lo, y = np.eye(m), np.ones(m), np.zeros((m, m)), np.zeros(m)
    info = C.c_int(0)
    return L.lib().arslam_debug_tile_llt(C.c_long(n), None if null_A else _dp(A), _dp(b), None, C.c_int(executor),
                                         _up(col_class), C.c_uint(flags), _dp(Lo), _dp(y), None, C.byref(info), None)


def _selinv(L, n):
    m = max(n, 1)
    A, Z = np.eye(m), np.zeros((m, m))
    info = C.c_int(0)
    return L.lib().arslam_debug_selinv(C.c_long(n), _dp(A), None, _dp(Z), None, C.byref(info))


def _tile_solve(L, n, nrhs):
    A, B = np.eye(n), np.ones((n, max(nrhs, 1)))
    X = np.zeros_like(B)
    info = C.c_int(0)
    return L.lib().arslam_debug_tile_solve(C.c_long(n), _dp(A), None, C.c_int(nrhs), _dp(B), _dp(X), C.byref(info))


def _residual_jacobian(L, n):
    m = max(n, 1)
    cam, cap, tag, corners = np.ones((m, 3)), np.zeros((m, 6)), np.zeros((m, 6)), np.zeros((m, 8))
    cap[:, 2] = 1.0
    r, J = np.zeros((m, 8)), np.zeros((m, 8, 15))
    return L.lib().arslam_debug_residual_jacobian(n, _dp(cam), _dp(cap), _dp(tag), _dp(corners), _dp(r), _dp(J))


def test_tile_llt_argument_checks(L):
    assert _tile_llt(L, 0) == E_INVALID_ARG
    assert _tile_llt(L, -3) == E_INVALID_ARG
    assert _tile_llt(L, 5, null_A=True) == E_INVALID_ARG
    assert _tile_llt(L, 5, executor=2) == E_INVALID_ARG
    assert _tile_llt(L, 5, executor=1, flags=2) == E_INVALID_ARG
    assert _tile_llt(L, 5, executor=0, flags=1) == E_INVALID_ARG                  # fill-first: executor 1 only
    assert _tile_llt(L, 5, executor=0, col_class=[0]) == E_INVALID_ARG            # two phases: likewise


def test_tile_llt_column_class_checks(L):
    assert _tile_llt(L, 5, executor=1, col_class=[2]) == E_INVALID_ARG            # classes are 0 / 1
    # n = 100: two tile columns, dense, so column 1 is column 0's parent
    assert _tile_llt(L, 100, executor=1, col_class=[1, 0]) == E_INVALID_ARG


def test_selinv_and_tile_solve_argument_checks(L):
    assert _selinv(L, 0) == E_INVALID_ARG
    assert _selinv(L, -1) == E_INVALID_ARG
    assert _tile_solve(L, 5, 0) == E_INVALID_ARG
    assert _tile_solve(L, 5, -2) == E_INVALID_ARG


def test_row_entry_argument_checks(L):
    assert _residual_jacobian(L, -1) == E_INVALID_ARG
    assert _residual_jacobian(L, 0) == OK
    cam, cap, tag, corners = np.ones((1, 3)), np.zeros((1, 6)), np.zeros((1, 6)), np.zeros((1, 8))
    r, J, rho = np.zeros((1, 8)), np.zeros((1, 8, 15)), np.zeros(1)
    for kind, a in ((9, 1.0), (L.LOSS_HUBER, 0.0), (L.LOSS_HUBER, float("nan"))):
        rc = L.lib().arslam_debug_residual_jacobian_loss(1, _dp(cam), _dp(cap), _dp(tag), _dp(corners),
                                                         _up([kind]), _dp(np.array([a])), _dp(r), _dp(J), _dp(rho))
        assert rc == E_INVALID_ARG, (kind, a)


def test_plan_probe_argument_checks(L, soa):
    lib = L.lib()
    facts = L.TilePlanFacts()
    assert lib.arslam_debug_tile_plan(0, None, None, None, C.byref(facts)) == E_INVALID_ARG
    assert lib.arslam_debug_tile_plan(-1, None, None, None, C.byref(facts)) == E_INVALID_ARG
    info = L.PlanInfo()
    assert lib.arslam_debug_reduced_plan(C.byref(soa.s), 3, 1, C.byref(info), None) == E_INVALID_ARG
    split = L.SplitInfo()
    assert lib.arslam_debug_rank_split(C.byref(soa.s), 2, 2, C.byref(split), None) == E_INVALID_ARG
    assert lib.arslam_debug_rank_split(C.byref(soa.s), 2, 5, C.byref(split), None) == E_INVALID_ARG
    n, dag_info = C.c_long(0), (C.c_int * 4)()
    assert lib.arslam_debug_dag_tasks(C.byref(soa.s), 1, 0, None, None, C.c_long(-1), C.byref(n),
                                      dag_info) == E_INVALID_ARG
    same, nd = C.c_int(0), C.c_int(0)
    assert lib.arslam_debug_gather_extend(C.byref(soa.s), C.c_int(soa.s.n_cap + 1), C.byref(same),
                                          C.byref(nd)) == E_INVALID_ARG


def test_schur_store_table_rejects_nblk_0_with_a_message(L):
    off, stored = np.zeros((13, 64, 4), np.int32), np.zeros((13, 64, 4), np.uint8)
    rc = L.lib().arslam_debug_schur_store_table(0, off.ctypes.data_as(C.POINTER(C.c_int)), _up(stored))
    assert rc == E_INVALID_ARG
    assert L.lib().arslam_lm_last_error().decode() != ""


def test_device_entries_answer_e_hip_without_a_device(L):
    if L.device_count() > 0:
        pytest.skip("a host without a HIP device only")
    assert _tile_llt(L, 5) == E_HIP
    assert _tile_llt(L, 5, executor=1) == E_HIP
    assert _selinv(L, 5) == E_HIP
    assert _tile_solve(L, 5, 3) == E_HIP
    assert _residual_jacobian(L, 1) == E_HIP
    assert _residual_jacobian(L, 0) == OK          # the process lives and still answers
