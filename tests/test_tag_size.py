"""CPU tests of per-tag side lengths: the reference the GPU tests lean on (tests/tag_size_ref.py)
and the host-side behaviour of the C-ABI that needs no device.

  * the scale identity r(f, t_c, w_c, t_t, w_t; s) = r_oracle(f, t_c / lam, w_c, t_t / lam, w_t),
    lam = s / 0.0635, against torch fp64 autograd of a restated projectCorner with a size: 1e-12
    relative to the row scale;
  * the dense LM of tag_size_ref at the default size against oracle.solve on every graph the GPU
    trace tests use, at the trace tolerances of tests/test_gpu_parity.py: per-iteration cost 1e-9
    for the first 5 iterations, final cost 1e-8, the same termination and rule, focal 1e-8;
  * argument validation, the handle's default side, the synthetic generator's sizes.
"""
import ctypes as C
import re

import numpy as np
import pytest

import tag_size_ref as ref
from ar_slam_amd import synth

INVALID_ARG = -1
BAD_SIZES = [0.0, -0.1, float("nan"), float("inf"), -float("inf")]
SIZES, tag_sizes, trace_graphs, arrays, assert_same_trace = (ref.SIZES, ref.tag_sizes, ref.trace_graphs, ref.arrays,
                                                              ref.assert_same_trace)


@pytest.fixture(scope="module")
def L():
    from ar_slam_amd import build, lm
    build.build()
    return lm


# ---- the reference ----

def _project_torch(torch, cam, cap, tag, size):
    """projectCorner (ar_slam_util.cpp:131-172) with a tag side, all four corners -> (8,)."""
    def rotate(w, p):
        th = torch.sqrt(torch.sum(w * w))
        u = w / th
        return p * torch.cos(th) + torch.linalg.cross(u, p) * torch.sin(th) + u * torch.dot(u, p) * (1 - torch.cos(th))
    out = []
    for d in synth.ARUCO_DIRECTIONS:
        c = torch.stack([0.5 * size * d[0], 0.5 * size * d[1], torch.zeros((), dtype=torch.float64)])
        a = rotate(tag[3:], c) + tag[:3] + cap[:3]
        p = rotate(cap[3:], a)
        out += [cam[0] * p[0] / p[2], cam[0] * p[1] / p[2]]
    return torch.stack(out)


def test_scale_identity_matches_autograd(oracle):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(17)
    worst = 0.0
    for i in range(48):
        size = (0.02, 0.0635, 0.15, 1.0)[i % 4]
        lam = size / ref.DEFAULT
        cam = np.array([rng.uniform(500, 3000), 0.0, 0.0])
        tag = np.concatenate([rng.normal(0, 1, 3) * lam, rng.normal(0, 1, 3)])
        cap = np.concatenate([-tag[:3] + (rng.normal(0, 0.2, 3) + [0, 0, 1.0]) * lam, rng.normal(0, 1, 3)])
        corners = rng.normal(0, 100, 8)
        r, J = ref.residual_jacobian(oracle, cam, cap, tag, corners, size)
        x = [torch.tensor(v, dtype=torch.float64) for v in (cam, cap, tag)]
        f = lambda a, b, c: _project_torch(torch, a, b, c, torch.tensor(size, dtype=torch.float64))   # noqa: E731
        proj = f(*x).numpy()
        Jt = np.concatenate([j.numpy() for j in torch.autograd.functional.jacobian(f, tuple(x))], 1)
        Jt[:, 1:3] = 0.0   # (l1, l2 take no part in the reference's projection)
        scale = np.abs(Jt).max(axis=1, keepdims=True)
        worst = max(worst, float(np.max(np.abs(J - Jt) / scale)),
                    float(np.max(np.abs(r - (proj - corners)) / np.maximum(np.abs(proj), 1.0))))
    print(f"identity against autograd: worst {worst:.2e}")
    assert worst <= 1e-12


def test_identity_is_the_oracle_at_the_default_size(oracle):
    rng = np.random.default_rng(2)
    cam, cap, tag, corners = np.array([900.0, 0, 0]), rng.normal(0, 1, 6), rng.normal(0, 1, 6), rng.normal(0, 100, 8)
    cap[:3] = -tag[:3] + [0, 0, 1.0]
    r, J = ref.residual_jacobian(oracle, cam, cap, tag, corners, ref.DEFAULT)
    ro, Jo = oracle.residual_jacobian(cam, cap, tag, corners)
    assert np.array_equal(r, ro) and np.array_equal(J, Jo)


@pytest.mark.parametrize("name", list(trace_graphs()))
def test_dense_lm_reproduces_the_oracle_at_the_default_size(oracle, name):
    g, camc, capc, tagc, _ = trace_graphs()[name]
    want = oracle.solve(*arrays(g), camera_const=camc, cap_const=capc, tag_const=tagc)
    ours = ref.solve(oracle, arrays(g), None, camc, capc, tagc)
    assert_same_trace(ours, want)
    assert want[3]["termination"] == "CONVERGENCE"


def test_dense_lm_is_scale_covariant(oracle):
    """A graph whose tags are all 0.20 m, solved with that side, follows the default-size solve
    of the same graph shrunk by lam: the same costs, the poses lam times larger.  (Jacobi scaling
    makes the step covariant; only the diagonal's clamp and the parameter tolerance see the scale.)"""
    g = synth.make_graph(6, 3, 2, seed=5, k=4)
    lam = 0.20 / ref.DEFAULT
    cap, tag = g.cap.copy(), g.tag.copy()
    cap[:, :3] *= lam
    tag[:, :3] *= lam
    big = ref.solve(oracle, (g.camera, cap, tag, g.obs_cap, g.obs_tag, g.corners), 0.20)
    small = ref.solve(oracle, arrays(g), None)
    cb = [it["cost"] for it in big[3]["iterations"]]
    cs = [it["cost"] for it in small[3]["iterations"]]
    assert len(cb) == len(cs)
    np.testing.assert_allclose(cb, cs, rtol=1e-6)
    np.testing.assert_allclose(big[2][:, :3], lam * small[2][:, :3], atol=1e-5)


# ---- the synthetic generator ----

def test_generator_default_is_unchanged_and_sizes_reach_the_corners():
    a = synth.make_graph(6, 3, 2, seed=5, k=4)
    b = synth.make_graph(6, 3, 2, seed=5, k=4, tag_size=synth.ARUCO_SIZE)
    assert np.array_equal(a.corners, b.corners) and np.array_equal(a.obs_tag, b.obs_tag)
    assert np.array_equal(a.cap, b.cap) and np.array_equal(a.tag, b.tag)
    sizes = np.array([0.03, 0.0635, 0.12, 0.30, 0.0635, 0.12])
    cap, tag = a.cap_true[a.obs_cap], a.tag_true[a.obs_tag]
    c = synth.project_corners(a.camera_true, cap, tag, sizes[a.obs_tag])
    assert np.array_equal(synth.project_corners(a.camera_true, cap, tag), synth.project_corners(a.camera_true, cap, tag, 0.0635))
    # the projected quad's extent grows with the side
    ext = np.ptp(c.reshape(-1, 4, 2), axis=1).max(1)
    ext0 = np.ptp(synth.project_corners(a.camera_true, cap, tag).reshape(-1, 4, 2), axis=1).max(1)
    np.testing.assert_allclose(ext / ext0, sizes[a.obs_tag] / 0.0635, rtol=0.15)


# ---- the C-ABI without a device ----

def test_exports(L):
    for name in ("arslam_lm_set_tag_size", "arslam_lm_get_tag_size", "arslam_lm_add_residual_block_sized",
                 "arslam_lm_load_soa_sized", "arslam_debug_residual_jacobian_sized"):
        assert name in L.EXPORTS
        assert hasattr(L.lib(), name), name
    assert L.DEFAULT_TAG_SIZE == ref.DEFAULT == synth.ARUCO_SIZE


def test_default_tag_size_of_a_handle(L):
    p = L.Problem()
    assert p.get_tag_size() == 0.0635
    p.set_tag_size(0.2)
    assert p.get_tag_size() == 0.2
    for bad in BAD_SIZES:
        with pytest.raises(L.LMError) as e:
            p.set_tag_size(bad)
        assert e.value.code == INVALID_ARG
        assert p.get_tag_size() == 0.2   # a rejected call leaves the handle as it was
    p.reset()
    assert p.get_tag_size() == 0.2       # reset keeps it, as it keeps the default loss
    assert L.lib().arslam_lm_get_tag_size(p._h, None) == INVALID_ARG
    assert L.lib().arslam_lm_set_tag_size(None, 0.1) == INVALID_ARG


def test_add_residual_block_rejects_a_bad_size(L):
    p = L.Problem()
    cam, cap, tag = np.array([900.0, 0, 0]), np.zeros(6), np.zeros(6)
    for bad in BAD_SIZES:
        with pytest.raises(L.LMError) as e:
            p.add_residual_block(np.zeros(8), cam, cap, tag, size=bad)
        assert e.value.code == INVALID_ARG
        assert p.num_residual_blocks() == 0
    p.add_residual_block(np.zeros(8), cam, cap, tag, size=0.3)
    p.add_residual_block(np.zeros(8), cam, cap, tag, size=0.3, loss=(L.LOSS_CAUCHY, 3.0))
    p.add_residual_block(np.zeros(8), cam, cap, tag)
    assert p.num_residual_blocks() == 3
    with pytest.raises(L.LMError) as e:
        p.add_residual_block(np.zeros(8), cam, cap, tag, size=0.3, loss=(L.LOSS_CAUCHY, -1.0))
    assert e.value.code == INVALID_ARG and p.num_residual_blocks() == 3


def test_load_soa_sized_rejects_a_bad_size_before_any_device_work(L):
    g = synth.make_graph(6, 3, 2, seed=5, k=4)
    for bad in BAD_SIZES:
        sizes = np.full(g.n_tag, 0.1)
        sizes[g.n_tag - 1] = bad
        with pytest.raises(L.LMError) as e:
            L.ResidentProblem(*arrays(g), tag_size=sizes)
        assert e.value.code == INVALID_ARG
    h = L.Problem()
    assert L.lib().arslam_lm_load_soa_sized(h._h, None, None, None, None) == INVALID_ARG


def test_debug_rows_reject_a_bad_size(L):
    z = np.zeros((1, 6))
    for bad in BAD_SIZES:
        with pytest.raises(L.LMError) as e:
            L.debug_residual_jacobian_sized(np.array([900.0, 0, 0]), z, z, np.zeros((1, 8)), bad)
        assert e.value.code == INVALID_ARG


def test_localizer_tag_size_validation(L):
    h = C.c_void_p()
    assert L.lib().arslam_localizer_create(C.byref(h), C.byref(L.make_options())) == 0
    try:
        s = C.c_double(-1.0)
        assert L.lib().arslam_localizer_get_tag_size(h, C.byref(s)) == 0 and s.value == 0.0635
        assert L.lib().arslam_localizer_set_tag_size(h, 0.25) == 0
        for bad in BAD_SIZES:
            assert L.lib().arslam_localizer_set_tag_size(h, bad) == INVALID_ARG
            assert L.lib().arslam_localizer_get_tag_size(h, C.byref(s)) == 0 and s.value == 0.25
        assert L.lib().arslam_localizer_get_tag_size(h, None) == INVALID_ARG
        # a bad side in a batch's array is rejected before any device work
        A = L._LocArrays(synth.LocalizeBatch(np.array([900.0, 0, 0]), np.zeros((2, 6)), np.array([0, 1], np.int32),
                                             np.array([0], np.int32), np.zeros((1, 8)), np.zeros((1, 6)), None),
                         True, None)
        for bad in BAD_SIZES:
            sizes = np.array([0.1, bad])
            assert L.lib().arslam_localizer_load_sized(h, C.byref(A.s), sizes.ctypes.data_as(L._dp), None,
                                                       None) == INVALID_ARG
    finally:
        L.lib().arslam_localizer_destroy(h)
    for name in ("arslam_localizer_set_tag_size", "arslam_localizer_get_tag_size", "arslam_localizer_load_sized",
                 "arslam_localize_many_sized"):
        assert name in L.EXPORTS and hasattr(L.lib(), name), name


def test_localize_batch_generator_default_is_unchanged():
    a = synth.make_localize_batch(map_name="small", n_query=8)
    b = synth.make_localize_batch(map_name="small", n_query=8, tag_size=synth.ARUCO_SIZE)
    assert np.array_equal(a.corners, b.corners) and np.array_equal(a.obs_tag, b.obs_tag)


# ---- the SLAM mirror's host side ----

def _fill(L, g, s=None):
    s = s or L.SlamSolver()
    for c in range(g.n_cap):
        sel = g.obs_cap == c
        s.add_detections(f"cap{c}", [f"tag_{t}" for t in g.obs_tag[sel]], g.corners[sel])
    return s


def test_mirror_sizes_by_id_and_default(L):
    g = synth.config_graph("tiny")
    s = L.SlamSolver()
    s.set_aruco_size(f"tag_{g.obs_tag[0]}", 0.30)        # before the tag's first detection
    _fill(L, g, s)
    ids = [s.aruco(a)[0] for a in range(s.num_arucos)]
    a0 = ids.index(f"tag_{g.obs_tag[0]}")
    assert s.aruco_size(a0) == 0.30
    assert all(s.aruco_size(a) == 0.0635 for a in range(s.num_arucos) if a != a0)
    s.set_aruco_size(ids[1], 0.12)                       # an existing, uninitialised tag
    assert s.aruco_size(1) == 0.12
    for bad in BAD_SIZES:
        for call in (lambda: s.set_aruco_size(ids[1], bad), lambda: s.set_default_aruco_size(bad)):
            with pytest.raises(L.LMError) as e:
                call()
            assert e.value.code == INVALID_ARG
    assert s.aruco_size(1) == 0.12
    s.set_default_aruco_size(0.2)
    s.add_detections("late", ["tag_new"], np.zeros((1, 8)))
    assert s.aruco_size(s.num_arucos - 1) == 0.2
    with pytest.raises(L.LMError):
        s.aruco_size(s.num_arucos)


def test_mirror_size_is_bound_once_the_tag_is_initialised(L):
    """solve() initialises the first capture's tags and adds their blocks before it needs a
    device; whether or not the solve then runs, those tags' sides are bound: STATE."""
    g = synth.config_graph("tiny")
    s = _fill(L, g)
    try:
        s.solve()
    except L.LMError:
        pass   # (no device here: the blocks were added all the same)
    bound = [a for a in range(s.num_arucos) if s.aruco(a)[2]]
    assert bound
    with pytest.raises(L.LMError) as e:
        s.set_aruco_size(s.aruco(bound[0])[0], 0.2)
    assert e.value.code == -7   # ARSLAM_E_STATE
    assert s.aruco_size(bound[0]) == 0.0635


def test_yaml_default_sizes_are_byte_identical_and_mixed_sizes_round_trip(L, tmp_path):
    g = synth.config_graph("tiny")
    rng = np.random.default_rng(1)
    poses = rng.normal(size=(64, 6))

    def filled(sizes=None, default=None):
        s = L.SlamSolver()
        if default is not None:
            s.set_default_aruco_size(default)
        for tid, v in (sizes or {}).items():
            s.set_aruco_size(tid, v)
        _fill(L, g, s)
        for a in range(s.num_arucos):
            s.set_aruco_pose(a, poses[a])
        return s
    plain, same = filled(), filled({f"tag_{g.obs_tag[0]}": 0.0635}, default=0.0635)
    plain.save_yaml(tmp_path / "a.yaml")
    same.save_yaml(tmp_path / "b.yaml")
    a_bytes = (tmp_path / "a.yaml").read_bytes()
    assert a_bytes == (tmp_path / "b.yaml").read_bytes()
    assert b"size" not in a_bytes
    sizes = {f"tag_{g.obs_tag[0]}": 0.30, f"tag_{g.obs_tag[1]}": 0.0301}
    mixed = filled(sizes)
    mixed.save_yaml(tmp_path / "m.yaml")
    assert (tmp_path / "m.yaml").read_bytes().count(b"    size: ") == 2
    t = L.SlamSolver()
    t.set_default_aruco_size(0.5)     # (an entry without the key is a 0.0635 m tag, whatever the loader's defaults)
    t.set_aruco_size(f"tag_{g.obs_tag[2]}", 0.7)
    t.load_yaml(tmp_path / "m.yaml")
    for a in range(mixed.num_arucos):
        assert t.aruco(a)[0] == mixed.aruco(a)[0]
        want = sizes.get(mixed.aruco(a)[0], 0.0635)
        assert t.aruco_size(a) == want
        np.testing.assert_array_equal(t.aruco(a)[1], mixed.aruco(a)[1])
    t.save_yaml(tmp_path / "m2.yaml")
    u = L.SlamSolver()
    u.load_yaml(tmp_path / "m2.yaml")
    assert [u.aruco_size(a) for a in range(u.num_arucos)] == [t.aruco_size(a) for a in range(t.num_arucos)]
    with pytest.raises(L.LMError):
        L.SlamSolver().load_yaml_string(re.sub(r"    size: \S+\n", "    size: -1\n", (tmp_path / "m.yaml").read_text(), count=1))


@pytest.mark.parametrize("size", [0.02, 0.0635, 0.15, 1.0])
def test_mirror_initialisers_match_the_oracle_through_the_identity(L, oracle, size):
    """calcInitValues / initArPose / initCapturePose with a side (arslam_slam_debug_init_pose, host
    only) against oracle.init_* with the pose translations scaled in and out: 1e-12 of the pose's
    scale; at 0.0635 the bits of the default-argument call."""
    rng = np.random.default_rng(23)
    lam = size / ref.DEFAULT
    worst = 0.0
    for i in range(64):
        camera = np.array([rng.uniform(500, 3000), 0.0, 0.0])
        rect = (rng.normal(0, 150, 2)[None] + 40.0 * rng.uniform(0.5, 2.0) *
                (synth.ARUCO_DIRECTIONS @ synth.rodrigues(np.array([0, 0, rng.uniform(-3, 3)]))[0, :2, :2].T) +
                rng.normal(0, 3.0, (4, 2))).reshape(8)
        pose = np.concatenate([rng.normal(0, 1, 3) * lam, rng.normal(0, 1, 3) * (0.0 if i % 7 == 0 else 1.0)])
        for which, want in (("ar", ref.init_ar_pose), ("capture", ref.init_capture_pose)):
            got = L.debug_slam_init_pose(which, rect, camera, pose, size)
            exp = want(oracle, rect, camera, pose, size)
            worst = max(worst, float(np.abs(got[:3] - exp[:3]).max() / max(np.abs(exp[:3]).max(), lam)),
                        float(np.abs(got[3:] - exp[3:]).max()))
            if size == 0.0635:
                assert np.array_equal(got, L.debug_slam_init_pose(which, rect, camera, pose))
                plain = (oracle.init_ar_pose if which == "ar" else oracle.init_capture_pose)(rect, camera, pose)
                np.testing.assert_allclose(got, plain, rtol=0, atol=1e-12 * max(1.0, np.abs(plain).max()))
            else:
                assert not np.allclose(got[:3], L.debug_slam_init_pose(which, rect, camera, pose)[:3], rtol=1e-3)
    print(f"initialisers at side {size}: worst {worst:.2e}")
    assert worst <= 1e-12
    for bad in BAD_SIZES[1:]:
        with pytest.raises(L.LMError):
            L.debug_slam_init_pose("ar", np.zeros(8), np.array([900.0, 0, 0]), np.zeros(6), bad)
