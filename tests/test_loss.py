"""Robust losses without a GPU: the numpy reference (tests/loss_ref.py) is
self-consistent, and the C-ABI validates its loss arguments on a handle that
never touches a device (arslam_lm_set_loss / get_loss /
add_residual_block_loss; include/arslam_lm.h).
"""
import numpy as np
import pytest

import loss_ref

KINDS = [loss_ref.NONE, loss_ref.HUBER, loss_ref.SOFT_L_ONE, loss_ref.CAUCHY]


@pytest.fixture(scope="module")
def L():
    from ar_slam_amd import build, lm
    build.build()
    return lm


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("a", [0.7, 3.0])
def test_rho_prime_is_the_derivative_of_rho(kind, a):
    """rho' against the central difference of rho at 200 values of s on both sides of a^2 (none
    within the difference step of Huber's kink), to 1e-6 relative."""
    b = a * a
    s = np.concatenate([np.geomspace(1e-3 * b, 0.99 * b, 100), np.geomspace(1.01 * b, 1e3 * b, 100)])
    h = 1e-6 * s
    num = (loss_ref.rho(kind, a, s + h)[0] - loss_ref.rho(kind, a, s - h)[0]) / (2 * h)
    p1 = loss_ref.rho(kind, a, s)[1]
    assert np.all(np.abs(num - p1) <= 1e-6 * np.abs(p1)), np.max(np.abs(num - p1) / np.abs(p1))
    # rho(0) = 0, rho'(0) = 1, rho' in (0, 1] and non-increasing (rho'' <= 0: the corrector's alpha = 0 branch)
    p0, p10 = loss_ref.rho(kind, a, 0.0)
    assert p0 == 0.0 and p10 == 1.0
    assert np.all(p1 > 0) and np.all(p1 <= 1.0) and np.all(np.diff(p1) <= 0)


@pytest.mark.parametrize("a", [0.7, 3.0, 1e6])
def test_huber_is_continuous_at_the_threshold(a):
    b = a * a
    lo, hi = np.nextafter(b, 0.0), np.nextafter(b, np.inf)
    (p_lo, d_lo), (p_at, d_at), (p_hi, d_hi) = (loss_ref.rho(loss_ref.HUBER, a, s) for s in (lo, b, hi))
    assert p_at == b and d_at == 1.0
    assert abs(p_hi - p_at) <= 4 * np.spacing(b) and abs(p_lo - p_at) <= 4 * np.spacing(b)
    assert abs(d_hi - 1.0) <= 4 * np.finfo(float).eps and d_lo == 1.0


def test_loss_constants_match_the_header(L):
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "arslam_lm.h")) as f:
        text = f.read()
    decl = dict(re.findall(r"(ARSLAM_LOSS_\w+) = (\d+)", text))
    assert decl == {"ARSLAM_LOSS_NONE": "0", "ARSLAM_LOSS_HUBER": "1", "ARSLAM_LOSS_SOFT_L_ONE": "2",
                    "ARSLAM_LOSS_CAUCHY": "3"}
    assert (L.LOSS_NONE, L.LOSS_HUBER, L.LOSS_SOFT_L_ONE, L.LOSS_CAUCHY) == (0, 1, 2, 3)
    assert (loss_ref.NONE, loss_ref.HUBER, loss_ref.SOFT_L_ONE, loss_ref.CAUCHY) == (0, 1, 2, 3)


BAD_SCALES = [0.0, -1.0, float("nan"), float("inf"), float("-inf")]


def test_set_loss_validates_and_a_rejected_call_changes_nothing(L):
    p = L.Problem()
    assert p.get_loss() == (L.LOSS_NONE, 0.0)
    p.set_loss(L.LOSS_HUBER, 3.0)
    assert p.get_loss() == (L.LOSS_HUBER, 3.0)
    for kind in (-1, 4, 5, 255, 1 << 20):
        with pytest.raises(L.LMError) as e:
            p.set_loss(kind, 1.0)
        assert e.value.code == -1
        assert p.get_loss() == (L.LOSS_HUBER, 3.0)
    for kind in (L.LOSS_HUBER, L.LOSS_SOFT_L_ONE, L.LOSS_CAUCHY):
        for a in BAD_SCALES:
            with pytest.raises(L.LMError) as e:
                p.set_loss(kind, a)
            assert e.value.code == -1
            assert p.get_loss() == (L.LOSS_HUBER, 3.0)
    for kind, a in ((L.LOSS_SOFT_L_ONE, 0.5), (L.LOSS_CAUCHY, 1e-3), (L.LOSS_HUBER, 1e300)):
        p.set_loss(kind, a)
        assert p.get_loss() == (kind, a)
    # NONE ignores its scale, whatever it is
    for a in BAD_SCALES + [7.0]:
        p.set_loss(L.LOSS_NONE, a)
        assert p.get_loss()[0] == L.LOSS_NONE


def test_add_residual_block_loss_validates_and_counts(L):
    p = L.Problem()
    cam, cap, tag = np.array([900.0, 0, 0]), np.zeros(6), np.zeros(6)
    tag2 = np.ones(6)
    rect = np.zeros(8)
    p.add_residual_block(rect, cam, cap, tag)
    p.add_residual_block(rect, cam, cap, tag2, loss=(L.LOSS_CAUCHY, 2.0))
    p.add_residual_block(rect, cam, cap, tag2, loss=(L.LOSS_NONE, float("nan")))   # NONE ignores a
    assert p.num_residual_blocks() == 3
    for loss in [(4, 1.0), (-1, 1.0)] + [(L.LOSS_HUBER, a) for a in BAD_SCALES]:
        with pytest.raises(L.LMError) as e:
            p.add_residual_block(rect, cam, cap, tag, loss=loss)
        assert e.value.code == -1
    assert p.num_residual_blocks() == 3   # a rejected block is not added
    assert p.get_loss() == (L.LOSS_NONE, 0.0)   # a block's own loss is not the default


def test_reset_keeps_the_default_loss(L):
    p = L.Problem()
    p.set_loss(L.LOSS_SOFT_L_ONE, 2.5)
    cam, cap, tag = np.array([900.0, 0, 0]), np.zeros(6), np.zeros(6)
    p.add_residual_block(np.zeros(8), cam, cap, tag)
    p.reset()
    assert p.num_residual_blocks() == 0
    assert p.get_loss() == (L.LOSS_SOFT_L_ONE, 2.5)


def test_load_soa_loss_rejects_bad_arrays_before_touching_a_device(L):
    """An invalid per-observation loss is an argument error (checked before the load starts a device)."""
    from ar_slam_amd import synth
    g = synth.config_graph("tiny")
    kinds = np.zeros(g.n_obs, np.uint8)
    a = np.ones(g.n_obs)
    kinds[3] = 9
    with pytest.raises(L.LMError) as e:
        L.ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, obs_loss=(kinds, a))
    assert e.value.code == -1
    kinds[3] = L.LOSS_HUBER
    a[3] = 0.0
    with pytest.raises(L.LMError) as e:
        L.ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, obs_loss=(kinds, a))
    assert e.value.code == -1
    with pytest.raises(ValueError):
        L.ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, obs_loss=(kinds[:-1], a[:-1]))


def test_load_soa_with_a_default_loss_rejects_negative_sizes(L):
    """The default loss is expanded per observation before the load: a negative n_obs is an argument
    error there too, not an allocation failure."""
    import ctypes as C
    from ar_slam_amd import synth
    g = synth.config_graph("tiny")
    p = L.Problem()
    p.set_loss(L.LOSS_HUBER, 3.0)
    A = L._Soa(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    A.s.n_obs = -1
    assert L.lib().arslam_lm_load_soa(p._h, C.byref(A.s)) == -1
    assert L.lib().arslam_lm_load_soa_loss(p._h, C.byref(A.s), None, None) == -1
