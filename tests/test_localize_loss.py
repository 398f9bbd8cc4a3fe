"""Robust losses of the batched localizer without a GPU: the numpy reference
(tests/localize_ref.py) is pinned to the oracle where they overlap (no loss),
the new entry points are exported, and the argument checks answer before any
device call (ARSLAM_E_INVALID_ARG on a host without a GPU, not NO_DEVICE).
"""
import ctypes as C

import numpy as np
import pytest

import localize_ref
import loss_ref
from ar_slam_amd import synth

INVALID_ARG = -1
NEW_SYMBOLS = ["arslam_localizer_set_loss", "arslam_localizer_get_loss", "arslam_localizer_load_loss",
               "arslam_localizer_observation_terms", "arslam_localize_many_loss",
               "arslam_slam_set_localize_loss"]


@pytest.fixture(scope="module")
def L():
    from ar_slam_amd import build, lm
    build.build()
    lm.lib()
    return lm


@pytest.fixture(scope="module")
def b4():
    return synth.make_localize_batch(n_query=4)


def test_reference_matches_oracle_without_a_loss(oracle):
    """Every kind NONE: the helper is the oracle's localize_many (status, iteration count, final
    cost 1e-9 relative, pose 1e-9)."""
    b = synth.make_localize_batch(n_query=64)
    ref = localize_ref.localize(oracle, b, kinds=loss_ref.NONE, scales=0.0)
    pose_o, status_o, sums_o = oracle.localize_many(b, with_summaries=True)
    np.testing.assert_array_equal(ref["status"], status_o)
    np.testing.assert_array_equal(ref["num_iterations"], [len(s["iterations"]) for s in sums_o])
    np.testing.assert_allclose(ref["final_cost"], [s["final_cost"] for s in sums_o], rtol=1e-9)
    np.testing.assert_allclose(ref["initial_cost"], [s["initial_cost"] for s in sums_o], rtol=1e-9)
    assert np.abs(ref["pose"] - pose_o).max() <= 1e-9
    s, w = ref["s"], ref["w"]
    assert (w == 1.0).all() and np.allclose(0.5 * s.reshape(64, 8).sum(1), ref["final_cost"], rtol=1e-12)


def test_new_symbols_are_exported(L):
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTS
        assert hasattr(L.lib(), name), name


def _handle(L):
    h = C.c_void_p()
    assert L.lib().arslam_localizer_create(C.byref(h), C.byref(L.make_options())) == 0
    return h


def _get(L, h):
    k, a = C.c_int(-5), C.c_double(-5.0)
    assert L.lib().arslam_localizer_get_loss(h, C.byref(k), C.byref(a)) == 0
    return k.value, a.value


@pytest.mark.parametrize("kind,a", [(4, 1.0), (-1, 1.0), (7, 1.0),
                                    (1, 0.0), (2, -1.0), (3, float("nan")), (1, float("inf")), (3, 0.0)])
def test_set_loss_rejects_bad_arguments(L, kind, a):
    h = _handle(L)
    try:
        assert _get(L, h) == (L.LOSS_NONE, 0.0)
        assert L.lib().arslam_localizer_set_loss(h, L.LOSS_HUBER, 2.5) == 0
        assert L.lib().arslam_localizer_set_loss(h, kind, a) == INVALID_ARG
        assert _get(L, h) == (L.LOSS_HUBER, 2.5)
        # NONE takes any scale (it is not read)
        assert L.lib().arslam_localizer_set_loss(h, L.LOSS_NONE, a) == 0
    finally:
        L.lib().arslam_localizer_destroy(h)


@pytest.mark.parametrize("case", ["kind_null", "scale_null", "bad_kind", "bad_scale", "nan_scale"])
def test_load_loss_rejects_bad_arrays(L, b4, case):
    """Checked before the device is touched: INVALID_ARG also where there is no GPU."""
    A = L._LocArrays(b4, True, None)
    kinds = np.full(A.s.n_obs, L.LOSS_CAUCHY, np.uint8)
    scales = np.full(A.s.n_obs, 3.0)
    kp, sp = kinds.ctypes.data_as(L._up), scales.ctypes.data_as(L._dp)
    if case == "kind_null":
        kp = None
    elif case == "scale_null":
        sp = None
    elif case == "bad_kind":
        kinds[5] = 4
    elif case == "bad_scale":
        scales[7] = 0.0
    else:
        scales[A.s.n_obs - 1] = np.nan
    h = _handle(L)
    try:
        assert L.lib().arslam_localizer_set_loss(h, L.LOSS_SOFT_L_ONE, 1.5) == 0
        assert L.lib().arslam_localizer_load_loss(h, C.byref(A.s), kp, sp) == INVALID_ARG
        assert _get(L, h) == (L.LOSS_SOFT_L_ONE, 1.5)
        # nothing was loaded: a solve and the terms still have no batch
        assert L.lib().arslam_localizer_solve(h, None, None, None) == -7
        assert L.lib().arslam_localizer_observation_terms(h, None, None) == -7
    finally:
        L.lib().arslam_localizer_destroy(h)


def test_localize_many_loss_rejects_bad_loss(L, b4):
    A = L._LocArrays(b4, True, None)
    res = (L.LocalizeResult * 4)()
    o = L.make_options()
    assert L.lib().arslam_localize_many_loss(C.byref(A.s), C.byref(o), 9, 1.0, res) == INVALID_ARG
    assert L.lib().arslam_localize_many_loss(C.byref(A.s), C.byref(o), L.LOSS_CAUCHY, -3.0, res) == INVALID_ARG
    assert (A.pose == 0.0).all()


def test_slam_mirror_rejects_bad_localize_loss(L):
    s = L.SlamSolver()
    try:
        assert L.lib().arslam_slam_set_localize_loss(s._h, 7, C.c_double(1.0)) == INVALID_ARG
        assert L.lib().arslam_slam_set_localize_loss(s._h, L.LOSS_HUBER, C.c_double(0.0)) == INVALID_ARG
        assert L.lib().arslam_slam_set_localize_loss(s._h, L.LOSS_CAUCHY, C.c_double(3.0)) == 0
        s.set_localize_loss(L.LOSS_NONE)
    finally:
        s.close()
