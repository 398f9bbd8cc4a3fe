"""CPU tests of the radial camera model: the reference the GPU tests lean on
(tests/distortion_ref.py) and the host-side behaviour that needs no device.

  * RadialOracle against central differences of its own residual on observations of the
    generator's geometry (r2 <= 0.5), step h = 1e-6 of the parameter's size: the rounding of the
    difference is eps |r| / h ~ 2e-16 x 500 / 1e-6 = 1e-7 against rows of scale 1e3 to 1e4, about
    1e-10 relative, and the truncation, h^2 / 6 times the third derivative, is below it: bound 1e-9;
  * at l1 = l2 = 0 against the oracle: the residual's bits, the Jacobian to 8 eps of its largest
    entry (the oracle's own Jacobian at f = 900 is the chain's at f = 1 times 900, a few roundings more);
  * the generator's option: None leaves a seed's graph as it is, the corners go through the model;
  * the handles' setters, the mirror's rules, the map file;
  * the README's scene solved by the dense LM of tag_size_ref with and without the model.
"""
import os

import numpy as np
import pytest

import distortion_ref as ref
import tag_size_ref
from ar_slam_amd import synth

INVALID_ARG, STATE = -1, -7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def L():
    from ar_slam_amd import build, lm
    build.build()
    return lm


# ---- the reference ----

def _draw(rng):
    cam = np.array([rng.uniform(500, 3000), 0.0, 0.0])
    tag = np.concatenate([rng.normal(0, 1, 3), rng.normal(0, 1, 3)])
    cap = np.concatenate([-tag[:3] + rng.normal(0, 0.2, 3) + [0, 0, 1.0], rng.normal(0, 1, 3)])
    return cam, cap, tag, rng.normal(0, 100, 8)


@pytest.mark.parametrize("l", [ref.MILD, ref.STRONG, (0.2, -0.05)])
def test_wrapper_matches_central_differences(oracle, l):
    R = ref.RadialOracle(oracle)
    g = ref.trace_graphs(ref.MILD)["g20"][0]      # (its geometry; the lens is the case's)
    worst = 0.0
    for o in range(0, g.n_obs, 5):
        cam, cap, tag, corners = g.camera.copy(), g.cap[g.obs_cap[o]], g.tag[g.obs_tag[o]], g.corners[o]
        cam[1:] = l
        r, J = R.residual_jacobian(cam, cap, tag, corners)
        assert np.array_equal(r, R.residual(cam, cap, tag, corners))
        assert np.all(J[:, 1:3] == 0.0)       # l1, l2 are held
        x = np.concatenate([cam, cap, tag])
        Jn = np.zeros((8, 15))
        for j in [0] + list(range(3, 15)):
            h = 1e-6 * max(1.0, abs(x[j]))
            xp, xm = x.copy(), x.copy()
            xp[j] += h
            xm[j] -= h
            Jn[:, j] = (R.residual(xp[:3], xp[3:9], xp[9:], corners) - R.residual(xm[:3], xm[3:9], xm[9:], corners)) / (xp[j] - xm[j])
        worst = max(worst, float(np.max(np.abs(J - Jn) / np.abs(J).max(axis=1, keepdims=True))))
    print(f"l = {l}: wrapper against central differences, worst {worst:.2e} of the row scale")
    assert worst <= 1e-9


def test_wrapper_is_the_oracle_without_distortion(oracle):
    R = ref.RadialOracle(oracle)
    rng = np.random.default_rng(2)
    worst = 0.0
    for _ in range(24):
        cam, cap, tag, corners = _draw(rng)
        cam[0] = 900.0
        r, J = R.residual_jacobian(cam, cap, tag, corners)
        ro, Jo = oracle.residual_jacobian(cam, cap, tag, corners)
        assert np.array_equal(r, ro) and np.array_equal(R.residual(cam, cap, tag, corners), ro)
        worst = max(worst, float(np.abs(J - Jo).max() / np.abs(Jo).max()))
    print(f"l = 0: Jacobian against the oracle's, worst {worst:.2e} of the largest entry")
    assert worst <= 8 * np.finfo(np.float64).eps


def test_wrapper_composes_with_the_sized_oracle(oracle):
    """SizedOracle over RadialOracle: the scale identity holds under the model."""
    R = ref.RadialOracle(oracle)
    rng = np.random.default_rng(5)
    cam, cap, tag, corners = _draw(rng)
    cam[1:] = ref.MILD
    lam = 0.20 / tag_size_ref.DEFAULT
    r0, J0 = R.residual_jacobian(cam, cap, tag, corners)
    cs, ts = cap.copy(), tag.copy()
    cs[:3] *= lam
    ts[:3] *= lam
    r1, J1 = tag_size_ref.SizedOracle(R, [0.20]).residual_jacobian(cam, cs, ts, corners)
    np.testing.assert_allclose(r1, r0, rtol=0, atol=1e-9)
    np.testing.assert_allclose(J1[:, 3:6] * lam, J0[:, 3:6], rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(J1[:, 6:9], J0[:, 6:9], rtol=1e-10, atol=1e-9)


# ---- the generator ----

def test_generator_default_is_unchanged_and_distortion_reaches_the_corners():
    a = synth.make_graph(6, 3, 2, seed=5, k=4)
    b = synth.make_graph(6, 3, 2, seed=5, k=4, distortion=None)
    for f in ("camera", "cap", "tag", "obs_cap", "obs_tag", "corners", "camera_true"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    z = synth.make_graph(6, 3, 2, seed=5, k=4, distortion=(0.0, 0.0))   # the model with a perfect lens
    assert np.array_equal(z.corners, a.corners)
    g = synth.make_graph(6, 3, 2, seed=5, k=4, distortion=ref.MILD, noise_px=0.0)
    assert np.array_equal(g.camera[1:], ref.MILD) and np.array_equal(g.camera_true, [synth.F_TRUE, *ref.MILD])
    cap, tag = g.cap_true[g.obs_cap], g.tag_true[g.obs_tag]
    pin = synth.project_corners(g.camera_true, cap, tag).reshape(-1, 2)
    r2 = np.sum((pin / synth.F_TRUE) ** 2, axis=1)
    want = pin * (1.0 + r2 * (ref.MILD[0] + ref.MILD[1] * r2))[:, None]
    np.testing.assert_allclose(g.corners.reshape(-1, 2), want, rtol=1e-13, atol=1e-10)
    # every detection is inside the image after the model, as the visibility test saw it
    assert np.all(np.abs(g.corners[:, 0::2]) < 0.5 * synth.IMG_W) and np.all(np.abs(g.corners[:, 1::2]) < 0.5 * synth.IMG_H)


def test_localize_batch_generator_default_is_unchanged():
    a = synth.make_localize_batch(map_name="tiny", n_query=8, k=4)
    b = synth.make_localize_batch(map_name="tiny", n_query=8, k=4, distortion=None)
    for f in ("camera", "tag", "q_start", "obs_tag", "corners", "pose_true"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    d = synth.make_localize_batch(map_name="tiny", n_query=8, k=4, distortion=ref.MILD)
    assert np.array_equal(d.camera[1:], ref.MILD)
    q_of = np.repeat(np.arange(8), 4)
    clean = synth.project_corners(d.camera, d.pose_true[q_of], d.tag[d.obs_tag], None, ref.MILD)
    assert np.abs(d.corners - clean).max() < 5.0          # (the 0.5 px noise, added after the model)
    assert np.abs(d.corners - synth.project_corners(d.camera, d.pose_true[q_of], d.tag[d.obs_tag])).max() > 5.0


# ---- the handles ----

def test_exports(L):
    for n in ("arslam_lm_set_camera_model", "arslam_lm_camera_model", "arslam_localizer_set_camera_model",
              "arslam_localizer_camera_model", "arslam_slam_set_camera_model", "arslam_slam_camera_model",
              "arslam_slam_camera_distortion", "arslam_debug_residual_jacobian_model"):
        assert n in L.EXPORTS and hasattr(L.lib(), n)
    assert (L.CAMERA_PINHOLE, L.CAMERA_RADIAL) == (0, 1)


def test_camera_model_of_a_mapper_handle(L):
    h = L.Problem()
    assert h.camera_model() == L.CAMERA_PINHOLE
    h.set_camera_model(L.CAMERA_RADIAL)
    assert h.camera_model() == L.CAMERA_RADIAL
    for bad in (-1, 2, 7):
        with pytest.raises(L.LMError) as e:
            h.set_camera_model(bad)
        assert e.value.code == INVALID_ARG
    assert h.camera_model() == L.CAMERA_RADIAL
    h.reset()                                   # (the model is the handle's, not the problem's)
    assert h.camera_model() == L.CAMERA_RADIAL
    assert L.lib().arslam_lm_camera_model(None, None) == INVALID_ARG


def test_debug_rows_reject_an_unknown_model(L):
    z = np.zeros((1, 6))
    with pytest.raises(L.LMError) as e:
        L.debug_residual_jacobian_model(np.zeros(3), z, z, np.zeros((1, 8)), 2)
    assert e.value.code == INVALID_ARG


# ---- the mirror ----

def _fill(L, g, s):
    for c in range(g.n_cap):
        sel = g.obs_cap == c
        s.add_detections(f"cap{c}", [f"tag_{t}" for t in g.obs_tag[sel]], g.corners[sel])
    return s


def test_mirror_model_rules_and_distortion_vector(L):
    g = synth.config_graph("tiny")
    s = L.SlamSolver()
    assert s.camera_model() == L.CAMERA_PINHOLE
    s.set_camera([900.0, -0.12, 0.03])
    assert np.array_equal(s.camera_distortion(), np.zeros(5))            # pinhole: l1, l2 take no part
    s.set_camera_model(L.CAMERA_RADIAL)
    assert s.camera_model() == L.CAMERA_RADIAL
    assert np.array_equal(s.camera_distortion(), [-0.12, 0.03, 0.0, 0.0, 0.0])
    with pytest.raises(L.LMError) as e:
        s.set_camera_model(5)
    assert e.value.code == INVALID_ARG and s.camera_model() == L.CAMERA_RADIAL
    _fill(L, g, s)
    s.set_camera_model(L.CAMERA_PINHOLE)        # detections alone bind nothing
    s.set_camera_model(L.CAMERA_RADIAL)
    try:
        s.solve()
    except L.LMError:
        pass   # (no device here: the first capture's blocks were added all the same)
    assert any(s.block(b)[3] for b in range(s.num_blocks))
    with pytest.raises(L.LMError) as e:
        s.set_camera_model(L.CAMERA_PINHOLE)
    assert e.value.code == STATE and s.camera_model() == L.CAMERA_RADIAL
    s.set_camera_model(L.CAMERA_RADIAL)         # (the model it has: nothing to refuse)


def _map(L, g, model=None, camera=(900.0, 0.0, 0.0)):
    rng = np.random.default_rng(1)
    poses = rng.normal(size=(64, 6))
    s = L.SlamSolver()
    if model is not None:
        s.set_camera_model(model)
    _fill(L, g, s)
    s.set_camera(camera)
    for a in range(s.num_arucos):
        s.set_aruco_pose(a, poses[a])
    return s


def test_yaml_pinhole_map_is_byte_identical_and_the_model_round_trips(L, tmp_path):
    g = synth.config_graph("tiny")
    plain, explicit = _map(L, g), _map(L, g, L.CAMERA_PINHOLE)
    plain.save_yaml(tmp_path / "a.yaml")
    explicit.save_yaml(tmp_path / "b.yaml")
    a_bytes = (tmp_path / "a.yaml").read_bytes()
    assert a_bytes == (tmp_path / "b.yaml").read_bytes() and b"model" not in a_bytes
    # what the parent of this change writes for the same store (tests/golden/distortion_pinhole_map.yaml)
    with open(os.path.join(GOLDEN, "distortion_pinhole_map.yaml"), "rb") as f:
        assert a_bytes == f.read()
    # a pinhole map that carries l1, l2 says nothing of a model either
    _map(L, g, camera=(900.0, -0.12, 0.03)).save_yaml(tmp_path / "c.yaml")
    assert b"model" not in (tmp_path / "c.yaml").read_bytes()
    radial = _map(L, g, L.CAMERA_RADIAL, camera=(900.0, -0.12, 0.03))
    radial.save_yaml(tmp_path / "r.yaml")
    text = (tmp_path / "r.yaml").read_text()
    assert text.count("  model: radial\n") == 1 and text.index("camera:") < text.index("  model: radial")
    t = L.SlamSolver()
    t.load_yaml(tmp_path / "r.yaml")
    assert t.camera_model() == L.CAMERA_RADIAL
    assert np.array_equal(t.camera_distortion(), [-0.12, 0.03, 0.0, 0.0, 0.0])
    t.save_yaml(tmp_path / "r2.yaml")
    assert (tmp_path / "r2.yaml").read_text() == text
    # an absent key and `pinhole` both mean the pinhole; anything else is an error
    u = L.SlamSolver()
    u.set_camera_model(L.CAMERA_RADIAL)
    u.load_yaml(tmp_path / "a.yaml")
    assert u.camera_model() == L.CAMERA_PINHOLE
    v = L.SlamSolver()
    v.load_yaml_string(text.replace("model: radial", "model: pinhole"))
    assert v.camera_model() == L.CAMERA_PINHOLE
    with pytest.raises(L.LMError):
        L.SlamSolver().load_yaml_string(text.replace("model: radial", "model: fisheye"))


# ---- the scene of the README ----

def test_scene_dense_lm_with_and_without_the_model(oracle):
    """The g20 graph at f = 900 on 1020 x 768 images through the lens distortion_ref.SCENE, solved
    by the dense LM with the model and as a pinhole (all any path could do before)."""
    g = ref.scene()
    cap, tag = g.cap_true[g.obs_cap], g.tag_true[g.obs_tag]
    pin = synth.project_corners(g.camera_true, cap, tag)
    shift = np.abs(synth.project_corners(g.camera_true, cap, tag, None, ref.SCENE) - pin).max()
    r2 = np.sum((pin.reshape(-1, 2) / synth.F_TRUE) ** 2, axis=1).max()
    A = tag_size_ref.arrays(g)
    radial = tag_size_ref.solve(ref.RadialOracle(oracle), A)
    pinhole = tag_size_ref.solve(oracle, A)
    rms_r, rms_p, f_r, f_p = ref.scene_figures(g, radial, pinhole)
    print(f"scene l = {ref.SCENE}: corner shift at most {shift:.1f} px, max r2 {r2:.2f}; dense LM with the model: "
          f"RMS {rms_r:.3f} px, f = {f_r:.1f}; as a pinhole: RMS {rms_p:.3f} px, f = {f_p:.1f} (truth 900)")
    assert radial[3]["termination"] == pinhole[3]["termination"] == "CONVERGENCE"
    ref.assert_scene(rms_r, rms_p, f_r, f_p)
