"""CPU tests of the estimated distortion (arslam_lm_set_estimate_distortion): the reference the
GPU tests lean on (tests/distortion_free_ref.py) and the host-side behaviour that needs no device.

  * FreeRadialOracle's two l columns against central differences of its own residual, on the
    geometry and at the bound of test_distortion.py's wrapper test (1e-9 of the row scale; the
    residual is linear in l1 and l2, so the difference has no truncation error at all);
  * the dense LM of tag_size_ref on the README's scene from l = (0, 0): it converges, to an RMS at
    most 0.75 of the pinhole's, and finds l1 within 0.02 of the lens's -0.14.  No bound on l2: 20
    captures do not pin it down;
  * the exports, the getter and setter, INVALID_ARG for values other than 0 and 1;
  * the switch does nothing on its own under CAMERA_PINHOLE.
"""
import numpy as np
import pytest

import distortion_free_ref as fref
import distortion_ref as ref
import tag_size_ref
from ar_slam_amd import synth

INVALID_ARG = -1


@pytest.fixture(scope="module")
def L():
    from ar_slam_amd import build, lm
    build.build()
    return lm


@pytest.mark.parametrize("l", [(0.0, 0.0), ref.MILD, ref.STRONG])
def test_l_columns_match_central_differences(oracle, l):
    R = fref.FreeRadialOracle(oracle)
    H = ref.RadialOracle(oracle)
    g = ref.trace_graphs(ref.MILD)["g20"][0]      # (its geometry; the lens is the case's)
    worst = 0.0
    for o in range(0, g.n_obs, 5):
        cam, cap, tag, corners = g.camera.copy(), g.cap[g.obs_cap[o]], g.tag[g.obs_tag[o]], g.corners[o]
        cam[1:] = l
        r, J = R.residual_jacobian(cam, cap, tag, corners)
        rh, Jh = H.residual_jacobian(cam, cap, tag, corners)
        assert np.array_equal(r, rh) and np.array_equal(r, R.residual(cam, cap, tag, corners))
        assert np.array_equal(np.delete(J, [1, 2], axis=1), np.delete(Jh, [1, 2], axis=1))   # the rest is the held model's
        Jn = np.zeros((8, 2))
        for a in range(2):
            h = 1e-6
            cp, cm = cam.copy(), cam.copy()
            cp[1 + a] += h
            cm[1 + a] -= h
            Jn[:, a] = (R.residual(cp, cap, tag, corners) - R.residual(cm, cap, tag, corners)) / (cp[1 + a] - cm[1 + a])
        worst = max(worst, float(np.max(np.abs(J[:, 1:3] - Jn) / np.abs(J).max(axis=1, keepdims=True))))
    print(f"l = {l}: l columns against central differences, worst {worst:.2e} of the row scale")
    assert worst <= 1e-9


def test_l_columns_compose_with_the_sized_oracle(oracle):
    """SizedOracle over FreeRadialOracle: x and y, and with them the two columns, do not change with the scale."""
    R = fref.FreeRadialOracle(oracle)
    g = ref.trace_graphs(ref.MILD)["g6"][0]
    cam, cap, tag, corners = g.camera.copy(), g.cap[g.obs_cap[0]], g.tag[g.obs_tag[0]], g.corners[0]
    lam = 0.20 / tag_size_ref.DEFAULT
    _, J0 = R.residual_jacobian(cam, cap, tag, corners)
    cs, ts = cap.copy(), tag.copy()
    cs[:3] *= lam
    ts[:3] *= lam
    _, J1 = tag_size_ref.SizedOracle(R, [0.20]).residual_jacobian(cam, cs, ts, corners)
    np.testing.assert_allclose(J1[:, 1:3], J0[:, 1:3], rtol=1e-10, atol=1e-9)
    assert np.abs(J0[:, 1]).max() > 1.0


def test_scene_dense_lm_finds_the_lens(oracle):
    g = ref.scene()
    A = tag_size_ref.arrays(g)
    free = tag_size_ref.solve(fref.FreeRadialOracle(oracle), fref.zero_lens(A))
    pinhole = tag_size_ref.solve(oracle, A)
    rms_f = synth.rms_px(free[3]["final_cost"], g.n_obs)
    rms_p = synth.rms_px(pinhole[3]["final_cost"], g.n_obs)
    print(f"scene l = {ref.SCENE}, dense LM from l = (0, 0): {len(free[3]['iterations'])} iterations, RMS {rms_f:.4f} px, "
          f"f = {free[0][0]:.2f}, l1 = {free[0][1]:.4f}, l2 = {free[0][2]:.4f}; as a pinhole RMS {rms_p:.4f} px, "
          f"f = {pinhole[0][0]:.2f}")
    assert free[3]["termination"] == "CONVERGENCE"
    assert rms_f <= 0.75 * rms_p
    assert abs(free[0][1] + 0.14) <= 0.02


def test_exports(L):
    for n in ("arslam_lm_set_estimate_distortion", "arslam_lm_estimate_distortion",
              "arslam_debug_residual_jacobian_distortion", "arslam_lm_debug_camera_rows"):
        assert n in L.EXPORTS and hasattr(L.lib(), n)


def test_switch_of_a_mapper_handle(L):
    h = L.Problem()
    assert h.estimate_distortion() is False
    h.set_estimate_distortion(True)
    assert h.estimate_distortion() is True
    for bad in (-1, 2, 7):
        with pytest.raises(L.LMError) as e:
            L._check(L.lib().arslam_lm_set_estimate_distortion(h._h, bad))
        assert e.value.code == INVALID_ARG
    assert h.estimate_distortion() is True          # a rejected call leaves the handle as it was
    h.reset()                                       # (the switch is the handle's, not the problem's)
    assert h.estimate_distortion() is True
    h.set_estimate_distortion(False)
    assert h.estimate_distortion() is False
    assert L.lib().arslam_lm_estimate_distortion(None, None) == INVALID_ARG
    assert L.lib().arslam_lm_set_estimate_distortion(None, 1) == INVALID_ARG


def test_switch_is_independent_of_the_camera_model(L):
    """Under PINHOLE the switch is kept and ignored: the model stays what it was, and model 2 stays invalid."""
    h = L.Problem()
    h.set_estimate_distortion(True)
    assert h.camera_model() == L.CAMERA_PINHOLE
    with pytest.raises(L.LMError) as e:
        h.set_camera_model(2)
    assert e.value.code == INVALID_ARG
    h.set_camera_model(L.CAMERA_RADIAL)
    assert h.estimate_distortion() is True and h.camera_model() == L.CAMERA_RADIAL
    h.set_camera_model(L.CAMERA_PINHOLE)
    assert h.estimate_distortion() is True
