"""GPU tests of per-tag side lengths in the LM solver, against tests/tag_size_ref.py.

The reference is exact per observation (the scale identity in tag_size_ref's header) and its
dense LM reproduces the oracle at the default side (tests/test_tag_size.py), so the tolerances
are the project's own:
  * rows: 1e-12 relative to the row scale, on the draws of tests/test_gpu_parity.py FILTERED to
    those whose four corners have |p_z| / |p| >= 4.5e-3 (the smallest ratio among that test's own
    512 draws is 4.57e-3; the filter reads the inputs only and drops about 1 draw in 100): every
    entry of a row carries 1 / p_z, whose relative error is eps |p| / |p_z| in any fp64 evaluation,
    so no fixed bound holds without a bound on that ratio (_random_obs); at 0.0635 the bits of
    debug_residual_jacobian;
  * LM traces: those of tests/test_gpu_parity.py (test_tag_size.assert_same_trace), and its pose
    check after one rigid gauge alignment;
  * pointer-keyed and appended problems against the SoA path / a fresh load: 1e-9;
  * the forced multi-rank path against one rank: the bounds of tests/test_gpu_multirank.py;
  * covariances: tol = 16 e_ref of the input, not below 1e-10, every block exactly symmetric
    (tests/test_gpu_lm_cov.py);
  * metric scale: the tag positions against the truth within 4x the dense reference's own error
    on the same input; without sizes the map comes out 0.0635 / 0.20 of the truth to 1e-3.
"""
import functools

import numpy as np
import pytest

import localize_ref
import tag_size_ref as ref
from ar_slam_amd import synth
from gauge import align_rigid, assert_poses_match
from loss_ref import CAUCHY
from tag_size_ref import arrays, assert_same_trace, tag_sizes, trace_graphs

pytestmark = pytest.mark.gpu

E_REF_CAP = 1e-9


MIN_DEPTH_RATIO = 4.5e-3


def _depth_ratio(cap, tag, size):
    """min over the four corners of |p_z| / |p|, p the corner in the camera frame."""
    n = len(cap)
    out = np.full(n, np.inf)
    for d in synth.ARUCO_DIRECTIONS:
        c = np.stack([0.5 * size * d[0], 0.5 * size * d[1], np.zeros(n)], 1)
        p = synth.angle_axis_rotate(cap[:, 3:], synth.angle_axis_rotate(tag[:, 3:], c) + tag[:, :3] + cap[:, :3])
        out = np.minimum(out, np.abs(p[:, 2]) / np.linalg.norm(p, axis=1))
    return out


def _random_obs(rng, n, size):
    """The draws of tests/test_gpu_parity.py (small angles, w = 0 exactly on every fifth tag),
    kept where every corner has |p_z| / |p| >= MIN_DEPTH_RATIO.  p_z comes out of a rotation's
    sum of terms of size |p|, so its relative error, and with it every entry of the row (all
    carry 1 / p_z), is about eps |p| / |p_z| in any fp64 evaluation: 1e-12 can only be asked where
    that ratio is bounded.  4.5e-3 is just below the smallest ratio among that test's own 512
    draws (4.57e-3), the conditioning its 1e-12 bound holds for; an unfiltered draw here reached
    8.7e-6."""
    m = 4 * n
    cam = np.stack([rng.uniform(500, 3000, m), np.zeros(m), np.zeros(m)], 1)
    tag = np.concatenate([rng.normal(0, 1, (m, 3)), rng.normal(0, 1, (m, 3))], 1)
    w = rng.normal(0, 1, (m, 3)) * rng.choice([1.0, 1e-2, 0.0, 3.0], (m, 1))
    cap = np.concatenate([-tag[:, :3] + rng.normal(0, 0.2, (m, 3)) + [0, 0, 1.0], w], 1)
    tag[::5, 3:] = 0.0
    corners = rng.normal(0, 100, (m, 8))
    size = np.resize(size, m)
    keep = np.nonzero(_depth_ratio(cap, tag, size) >= MIN_DEPTH_RATIO)[0][:n]
    assert len(keep) == n
    assert (np.sum(tag[keep, 3:] ** 2, 1) == 0).sum() >= n // 8 and (np.sum(cap[keep, 3:] ** 2, 1) < 1e-3).sum() >= n // 8
    return cam[keep], cap[keep], tag[keep], corners[keep], size[keep]


# ---- 1. rows ----

def test_sized_rows_match_the_identity(lm, oracle):
    rng = np.random.default_rng(7)
    n = 256
    cam, cap, tag, corners, size = _random_obs(rng, n, [0.02, 0.0635, 0.15, 1.0])
    assert all((size == v).sum() >= n // 8 for v in (0.02, 0.0635, 0.15, 1.0))
    r, J = lm.debug_residual_jacobian_sized(cam, cap, tag, corners, size)
    worst = 0.0
    for i in range(n):
        ro, Jo = ref.residual_jacobian(oracle, cam[i], cap[i], tag[i], corners[i], size[i])
        np.testing.assert_allclose(r[i], ro, rtol=1e-12, atol=1e-9)
        scale = np.abs(Jo).max(axis=1, keepdims=True) + 1e-300
        worst = max(worst, float(np.max(np.abs(J[i] - Jo) / scale)))
    print(f"sized rows: worst Jacobian error {worst:.2e} of the row scale")
    assert worst < 1e-12
    assert np.array_equal(J[..., 3:6], J[..., 9:12])
    # at the default side: the bits of the constant-size entry
    r0, J0 = lm.debug_residual_jacobian(cam, cap, tag, corners)
    rd, Jd = lm.debug_residual_jacobian_sized(cam, cap, tag, corners, 0.0635)
    assert np.array_equal(r0, rd) and np.array_equal(J0, Jd)
    d = size == 0.0635
    assert np.array_equal(r[d], r0[d]) and np.array_equal(J[d], J0[d])


# ---- 2. the default is untouched ----

def _trace(s):
    return [(it["cost"], it["gradient_max_norm"], it["step_norm"], it["trust_region_radius"]) for it in s["iterations"]]


@pytest.mark.parametrize("loss", [None, (CAUCHY, 3.0)], ids=["plain", "cauchy"])
def test_default_sizes_are_bit_identical(lm, loss):
    g = trace_graphs()["gk11"][0]   # (the one-chunk and the chunked instances; detections of default-size tags)
    a = lm.ResidentProblem(*arrays(g), loss=loss)
    b = lm.ResidentProblem(*arrays(g), loss=loss, tag_size=np.full(g.n_tag, 0.0635))
    c = lm.ResidentProblem(*arrays(g), loss=loss, tag_size=0.0635)
    sa, sb, sc = a.solve(), b.solve(), c.solve()
    for s, p in ((sb, b), (sc, c)):
        assert _trace(s) == _trace(sa)
        assert np.array_equal(p.camera, a.camera) and np.array_equal(p.cap, a.cap) and np.array_equal(p.tag, a.tag)


def test_set_tag_size_drops_a_loaded_problem_and_sizes_a_later_load(lm, oracle):
    g = trace_graphs()["g6"][0]
    rp = lm.ResidentProblem(*arrays(g))
    rp.solve()
    rp.set_tag_size(0.12)
    with pytest.raises(lm.LMError) as e:
        rp.solve()
    assert e.value.code == -7   # ARSLAM_E_STATE: nothing loaded
    # the handle's default sizes every tag of a later load
    h = lm.Problem()
    h.set_tag_size(0.12)
    camera, caps, tags = g.camera.copy(), [c.copy() for c in g.cap], [t.copy() for t in g.tag]
    for b in range(g.n_obs):
        h.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]])
    s = h.solve()
    u = lm.ResidentProblem(*arrays(g), tag_size=0.12)
    su = u.solve()
    assert abs(s["initial_cost"] - su["initial_cost"]) <= 1e-12 * su["initial_cost"]
    want = ref.terms(oracle, arrays(g), 0.12).cost
    assert abs(su["initial_cost"] - want) <= 1e-9 * want


# ---- 3. traces against the dense LM ----

def _losses(g, with_loss):
    if not with_loss:
        return None
    return np.full(g.n_obs, CAUCHY, np.uint8), np.full(g.n_obs, 3.0)


@functools.lru_cache(maxsize=None)
def _dense(oracle, name, with_loss):
    g, camc, capc, tagc, sizes = trace_graphs(sized=True)[name]
    kinds, a = (CAUCHY, 3.0) if with_loss else (0, 0.0)
    return ref.solve(oracle, arrays(g), sizes, camc, capc, tagc, kinds, a)


def _check_trace(lm, oracle, name, with_loss, **opts):
    g, camc, capc, tagc, sizes = trace_graphs(sized=True)[name]
    assert len(np.unique(sizes)) > 1
    want = _dense(oracle, name, with_loss)
    rp = lm.ResidentProblem(*arrays(g), camc, capc, tagc, obs_loss=_losses(g, with_loss), tag_size=sizes, **opts)
    s = rp.solve()
    ours = (rp.camera, rp.cap, rp.tag, s)
    assert_same_trace(ours, want)
    assert_poses_match(ours[1], ours[2], want[1], want[2], tags=np.unique(g.obs_tag), caps=np.unique(g.obs_cap))
    assert s["termination"] == "CONVERGENCE"
    return s


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
@pytest.mark.parametrize("name", ["g6", "g20", "gk11", "g20_tag_const", "g20_cap_const", "g20_camera_const"])
def test_mixed_size_trace_matches_the_dense_lm(lm, oracle, name, with_loss):
    _check_trace(lm, oracle, name, with_loss)


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
@pytest.mark.parametrize("side", ["ELIM_CAPTURES", "ELIM_TAGS", "ELIM_MIXED"])
def test_mixed_size_trace_under_every_elimination(lm, oracle, side, with_loss):
    s = _check_trace(lm, oracle, "small", with_loss, elimination=getattr(lm, side))
    assert s["elimination_used"] == getattr(lm, side)


# ---- 4. the pointer-keyed API ----

def _add(prob, g, sizes, camera, caps, tags, blocks, loss=None):
    for b in blocks:
        prob.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]], loss=loss,
                                size=sizes[g.obs_tag[b]])


def test_pointer_keyed_sizes_match_the_soa_path(lm):
    g, _, _, _, sizes = trace_graphs(sized=True)["g20"]
    camera, caps, tags = g.camera.copy(), [c.copy() for c in g.cap], [t.copy() for t in g.tag]
    prob = lm.Problem()
    _add(prob, g, sizes, camera, caps, tags, range(g.n_obs))
    s = prob.solve()
    rp = lm.ResidentProblem(*arrays(g), tag_size=sizes)
    s2 = rp.solve()
    assert (s["termination"], s["rule"]) == (s2["termination"], s2["rule"])
    assert len(s["iterations"]) == len(s2["iterations"])
    for a, b in zip(s["iterations"], s2["iterations"]):
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"]
    assert abs(camera[0] - rp.camera[0]) <= 1e-9 * rp.camera[0]


def test_appended_sized_blocks_keep_the_plan_and_match_a_fresh_load(lm):
    sizes = tag_sizes(300)
    g = synth.config_graph("cfg2", tag_size=sizes)   # (as tests/test_gpu_parity.py's append test)
    camera, caps, tags = g.camera.copy(), [c.copy() for c in g.cap], [t.copy() for t in g.tag]
    prob = lm.Problem(elimination=lm.ELIM_CAPTURES)
    first = 700
    _add(prob, g, sizes, camera, caps, tags, np.nonzero(g.obs_cap < first)[0])
    s1 = prob.solve()
    assert s1["setup_kind"] == lm.SETUP_LOAD
    seen = set(g.obs_tag[g.obs_cap < first].tolist())
    pairs = set()
    for c in range(first):
        ts = sorted(set(g.obs_tag[g.obs_cap == c].tolist()))
        pairs.update((a, b) for a in ts for b in ts if a < b)
    added = []
    for c in range(first, g.n_cap):
        ts = sorted(set(g.obs_tag[g.obs_cap == c].tolist()))
        if set(ts) <= seen and all((a, b) in pairs for a in ts for b in ts if a < b):
            added.append(c)
    added = added[:20]
    assert len(added) >= 5
    for c in added:
        _add(prob, g, sizes, camera, caps, tags, np.nonzero(g.obs_cap == c)[0])
    start = (camera.copy(), [c.copy() for c in caps], [t.copy() for t in tags])
    s2 = prob.solve()
    assert s2["setup_kind"] == lm.SETUP_APPEND, s2["setup_kind"]
    fresh = lm.Problem(elimination=lm.ELIM_CAPTURES)
    cam_f, caps_f, tags_f = start[0].copy(), [c.copy() for c in start[1]], [t.copy() for t in start[2]]
    _add(fresh, g, sizes, cam_f, caps_f, tags_f, np.nonzero(g.obs_cap < first)[0])
    for c in added:
        _add(fresh, g, sizes, cam_f, caps_f, tags_f, np.nonzero(g.obs_cap == c)[0])
    s3 = fresh.solve()
    assert [i["step_is_successful"] for i in s2["iterations"]] == [i["step_is_successful"] for i in s3["iterations"]]
    for a, b in zip(s2["iterations"], s3["iterations"]):
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"]
    assert abs(camera[0] - cam_f[0]) <= 1e-8 * cam_f[0]
    # the sizes took part: the same blocks at the default side start from another cost
    plain = lm.Problem(elimination=lm.ELIM_CAPTURES)
    cam_p, caps_p, tags_p = start[0].copy(), [c.copy() for c in start[1]], [t.copy() for t in start[2]]
    _add(plain, g, np.full(g.n_tag, 0.0635), cam_p, caps_p, tags_p, np.nonzero(g.obs_cap < first)[0])
    assert abs(plain.solve()["initial_cost"] - s1["initial_cost"]) > 1e-3 * s1["initial_cost"]


# ---- 5. several ranks ----

def test_forced_multirank_path_carries_the_sizes(lm):
    sizes = tag_sizes(80)
    g = synth.config_graph("medium", tag_size=sizes)
    plain = lm.ResidentProblem(*arrays(g), tag_size=sizes)
    sp = plain.solve()
    multi = lm.ResidentProblem(*arrays(g), tag_size=sizes, comm=(0, 1, lambda a, op: None), force_multirank=True)
    sm = multi.solve()
    assert sm["comm_calls"] > 0 and sp["comm_calls"] == 0
    assert (sm["termination"], sm["rule"]) == (sp["termination"], sp["rule"])
    assert len(sm["iterations"]) == len(sp["iterations"])
    for a, b in zip(sm["iterations"], sp["iterations"]):
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * abs(b["cost"])
    np.testing.assert_allclose([i["trust_region_radius"] for i in sm["iterations"]],
                               [i["trust_region_radius"] for i in sp["iterations"]], rtol=1e-9)
    assert abs(multi.camera[0] - plain.camera[0]) <= 1e-8 * plain.camera[0]
    assert_poses_match(multi.cap, multi.tag, plain.cap, plain.tag)


# ---- 6. the localizer ----

LOC_FIELDS = ["status", "rule", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "init_obs",
              "initial_cost", "final_cost"]


def _rot_err(w1, w2):
    R1, R2 = synth.rodrigues(w1), synth.rodrigues(w2)
    return np.arccos(np.clip((np.einsum("nij,nij->n", R1, R2) - 1.0) / 2.0, -1.0, 1.0))


@pytest.fixture(scope="module")
def sized96():
    """96 queries against the 80-tag map of "medium" with one side per tag drawn from SIZES, and
    the same with one detection per query shifted 40 px."""
    sizes = tag_sizes(80)
    b = synth.make_localize_batch(map_name="medium", n_query=96, tag_size=sizes)
    b.tag_in_map = np.ones(len(sizes), np.uint8)
    b.tag_in_map[b.obs_tag[b.q_start[9]]] = 0    # query 9 initialises from a later block
    return sizes, b, localize_ref.shifted_batch(b, seed=11, px=40.0)[0]


def test_default_sizes_are_bit_identical_in_the_localizer(lm):
    b = synth.make_localize_batch(map_name="medium", n_query=96)
    p0, r0, _ = lm.Localizer(b).solve()
    p1, r1, _ = lm.Localizer(b, tag_size=np.full(b.tag.shape[0], 0.0635)).solve()
    p2, r2 = lm.localize_many(b, tag_size=0.0635)
    for p, r in ((p1, r1), (p2, r2)):
        assert np.array_equal(p, p0)
        for f in LOC_FIELDS:
            np.testing.assert_array_equal(r[f], r0[f], err_msg=f)


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
@pytest.mark.parametrize("init_from_map", [1, 0])
def test_sized_localizer_matches_numpy(lm, oracle, sized96, init_from_map, with_loss):
    sizes, clean, shifted = sized96
    b = shifted if with_loss else clean
    kinds, scales = ((CAUCHY, 3.0) if with_loss else (None, None))
    pose0 = None if init_from_map else b.pose_true + 0.01
    want = ref.localize(oracle, b, sizes, kinds, scales, init_from_map=bool(init_from_map), pose=pose0)
    loc = lm.Localizer(b, init_from_map=bool(init_from_map), pose=pose0, tag_size=sizes,
                       loss=(CAUCHY, 3.0) if with_loss else None)
    pose, res, _ = loc.solve()
    ok = want["status"] >= 0
    assert ok.all()
    for f in ("status", "rule", "num_iterations", "init_obs"):
        np.testing.assert_array_equal(res[f], want[f], err_msg=f)
    assert res["init_obs"][9] == b.q_start[9] + 1
    d_t = np.abs(pose[:, :3] - want["pose"][:, :3]).max()
    d_r = _rot_err(pose[:, 3:], want["pose"][:, 3:]).max()
    print(f"96 queries: translation {d_t:.2e} m, rotation {d_r:.2e} rad, final cost "
          f"{np.abs(res['final_cost'] / want['final_cost'] - 1.0).max():.2e} rel")
    np.testing.assert_allclose(res["final_cost"], want["final_cost"], rtol=1e-8)
    np.testing.assert_allclose(res["initial_cost"], want["initial_cost"], rtol=1e-12 if not init_from_map else 1e-9)
    assert d_t < 1e-7 and d_r < 1e-7
    # the sizes took part: the poses are the truth's, not a shrunken map's
    assert np.abs(pose[:, :3] - b.pose_true[:, :3]).max() < 0.05
    # observation_terms and covariance on the same batch, at the device's poses
    s, w = loc.observation_terms()
    s_ref, w_ref = localize_ref.observation_terms(ref.MapSizedOracle(oracle, b.tag, sizes), b, pose, kinds, scales,
                                                  res["status"])
    np.testing.assert_allclose(s, s_ref, rtol=1e-12)
    np.testing.assert_allclose(w, w_ref, rtol=1e-12)
    cov, st, mp = loc.covariance()
    c_ref, s_st, m_ref = ref.localize_covariance(oracle, b, sizes, pose, kinds, scales, res["status"], res["rule"])
    np.testing.assert_array_equal(st, s_st)
    assert (m_ref >= 1e-4).all(), m_ref.min()      # the 1e-9 below rests on this (tests/test_gpu_localize_cov.py)
    d = np.sqrt(np.einsum("qii->qi", c_ref))
    err = (np.abs(cov - c_ref) / (d[:, :, None] * d[:, None, :])).max()
    print(f"covariance {err:.2e} relative to sqrt(C_ii C_jj), min_pivot {np.abs(mp - m_ref).max():.2e} absolute")
    assert err <= 1e-9
    assert np.abs(mp - m_ref).max() <= 1e-12
    np.testing.assert_array_equal(cov, cov.transpose(0, 2, 1))
    # the one-shot entry: the resident handle's bits
    p1, r1 = lm.localize_many(b, init_from_map=bool(init_from_map), pose=pose0, tag_size=sizes,
                              loss=(CAUCHY, 3.0) if with_loss else None)
    assert np.array_equal(p1, pose)


# ---- 7. covariance ----

def _cov_check(lm, oracle, g, sizes, elimination):
    tc = np.zeros(g.n_tag, np.uint8)
    tc[0] = 1
    rp = lm.ResidentProblem(*arrays(g), tag_const=tc, tag_size=sizes, elimination=elimination)
    s = rp.solve()
    assert s["elimination_used"] == elimination
    out = rp.covariance()
    at = (rp.camera, rp.cap, rp.tag, g.obs_cap, g.obs_tag, g.corners)
    want = ref.covariance(oracle, at, sizes, tag_const=tc, scale_arrays=arrays(g))
    assert want.e_ref <= E_REF_CAP
    tol = max(16.0 * want.e_ref, 1e-10)
    assert out["info"]["status"] == lm.COV_OK
    assert np.array_equal(out["cap_status"], want.cap_status) and np.array_equal(out["tag_status"], want.tag_status)
    worst = abs(out["var_f"] - want.var_f) / want.var_f
    for dev, w, st in ((out["cap"], want.cap, want.cap_status), (out["tag"], want.tag, want.tag_status)):
        ok = st == 0
        assert np.array_equal(dev[ok], np.transpose(dev[ok], (0, 2, 1)))
        d = np.sqrt(np.einsum("bii->bi", w[ok]))
        worst = max(worst, float(np.max(np.abs(dev[ok] - w[ok]) / (d[:, :, None] * d[:, None, :]))))
    print(f"covariance error {worst:.2e} (tol {tol:.2e}, e_ref {want.e_ref:.2e})")
    assert worst <= tol
    return rp, out, want, at, tc


@pytest.mark.parametrize("side", ["ELIM_CAPTURES", "ELIM_TAGS"])
def test_covariance_of_a_mixed_size_graph(lm, oracle, side):
    g, _, _, _, sizes = trace_graphs(sized=True)["g20"]
    rp, out, want, at, tc = _cov_check(lm, oracle, g, sizes, getattr(lm, side))
    T, Cp, Cm = lm.BLOCK_TAG, lm.BLOCK_CAPTURE, lm.BLOCK_CAMERA
    pairs = [((T, 1), (T, g.n_tag - 1)), ((T, 2), (T, 3)), ((Cp, 0), (T, 5)), ((T, 5), (Cp, 0)), ((Cp, 1), (Cp, 7)),
             ((Cm, 0), (T, 4)), ((Cp, 2), (Cm, 0)), ((T, 6), (T, 6)), ((T, 0), (T, 1))]
    cov, st, _ = rp.covariance_pairs(pairs)
    pw = ref.covariance_pairs(oracle, at, sizes, pairs, tag_const=tc, scale_arrays=arrays(g))
    assert np.array_equal(st, pw.status)
    tol = max(16.0 * max(pw.e_ref_pairs, want.e_ref), 1e-10)
    worst = 0.0
    for p in range(len(pairs)):
        if pw.status[p] != 0:
            assert np.all(cov[p] == -1.0)
            continue
        worst = max(worst, float(np.max(np.abs(cov[p] - pw.cov[p]) / pw.scale[p])))
    print(f"pairs error {worst:.2e} (tol {tol:.2e})")
    assert worst <= tol
    assert np.array_equal(cov[2], cov[3].T)        # (a, b) and (b, a): transposes of the same bits
    assert np.array_equal(cov[7], cov[7].T)


# ---- 8. metric scale ----

def _similarity_scale(P, Q):
    """s of the best-fit similarity Q ~ s R P + t (Umeyama)."""
    Pc, Qc = P - P.mean(0), Q - Q.mean(0)
    U, D, Vt = np.linalg.svd(Qc.T @ Pc / len(P))
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    return float(np.trace(np.diag(D) @ S) / (np.sum(Pc * Pc) / len(P)))


def test_metric_scale_comes_from_the_tag_size(lm, oracle):
    """Tags of 0.20 m.  With tag_size the map is metric: the tag positions match the truth, after
    a rigid alignment with no scale, as well as the dense reference's do.  Without, the same
    detections give a map 0.0635 / 0.20 the size of the truth (started from the initial state
    shrunk by that factor, as the initialisers would start it)."""
    g = synth.make_graph(20, 5, 4, seed=5, k=6, noise_px=0.5, tag_size=0.20, depth=(1.5, 2.5))
    tc = np.zeros(g.n_tag, np.uint8)
    tc[0] = 1
    truth = g.tag_true[:, :3]
    want = ref.solve(oracle, arrays(g), 0.20, tag_const=tc)
    e_ref = float(np.abs(align_rigid(want[2][:, :3], truth) - truth).max())
    rp = lm.ResidentProblem(*arrays(g), tag_const=tc, tag_size=0.20)
    s = rp.solve()
    e_dev = float(np.abs(align_rigid(rp.tag[:, :3], truth) - truth).max())
    scale_sized = _similarity_scale(truth, rp.tag[:, :3])
    lam = 0.0635 / 0.20
    cap, tag = g.cap.copy(), g.tag.copy()
    cap[:, :3] *= lam
    tag[:, :3] *= lam
    un = lm.ResidentProblem(g.camera, cap, tag, g.obs_cap, g.obs_tag, g.corners, tag_const=tc)
    su = un.solve()
    scale_unsized = _similarity_scale(truth, un.tag[:, :3])
    print(f"0.20 m tags: largest tag position error {1e3 * e_dev:.3f} mm with tag_size (dense reference "
          f"{1e3 * e_ref:.3f} mm, similarity scale {scale_sized:.5f}); without sizes the map's scale is "
          f"{scale_unsized:.5f} of the truth (0.0635 / 0.20 = {lam:.5f})")
    assert s["termination"] == su["termination"] == "CONVERGENCE"
    assert e_dev <= 4.0 * e_ref
    assert abs(scale_unsized - lam) <= 1e-3


# ---- 9. printed figures ----

def test_printed_figures_large_anchor(lm, oracle):
    """The README's 60-capture / 60-tag graph at 0.5 px with its anchor, tag 0, 0.30 m instead of
    0.0635 m: the 1-sigma tag positions beside the 37.5 / 66.4 mm of the 6 cm anchor.  The graph
    is the README's own -- the same captures, detections and noise draws -- with the two
    detections of tag 0 projected from a 0.30 m tag.  Asserted: agreement with the dense reference
    only; the improvement is a figure to report."""
    import dataclasses
    sizes = np.full(60, 0.0635)
    sizes[0] = 0.30
    g = synth.make_graph(60, 10, 6, seed=7, k=8)
    cap, tag = g.cap_true[g.obs_cap], g.tag_true[g.obs_tag]
    noise = g.corners - synth.project_corners(g.camera_true, cap, tag)
    g = dataclasses.replace(g, corners=synth.project_corners(g.camera_true, cap, tag, sizes[g.obs_tag]) + noise)
    rp, out, want, _, _ = _cov_check(lm, oracle, g, sizes, lm.ELIM_CAPTURES)
    ok = out["tag_status"] == lm.COV_OK
    pos = 0.5 * np.sqrt(np.einsum("bii->b", out["tag"][ok][:, :3, :3]))
    okr = want.tag_status == 0
    pos_ref = 0.5 * np.sqrt(np.einsum("bii->b", want.tag[okr][:, :3, :3]))
    print(f"60 tags, 60 captures, 0.5 px, anchor tag 0.30 m: 1-sigma tag position median {1e3 * np.median(pos):.2f} mm, "
          f"largest {1e3 * pos.max():.2f} mm (dense reference {1e3 * np.median(pos_ref):.2f} / {1e3 * pos_ref.max():.2f} mm; "
          f"6 cm anchor: 37.5 / 66.4 mm); sigma_f {0.5 * np.sqrt(out['var_f']):.3f} px")
    assert np.all(pos > 0)


# ---- 10. the SLAM mirror ----

def _mirror_scene():
    """10 captures of an 8-tag wall (4 x 2), 6 tags each, one side per tag drawn from SIZES;
    2 more captures held out for localize_many."""
    sizes = tag_sizes(8, seed=4)
    assert len(np.unique(sizes)) > 1
    g = synth.make_graph(12, 4, 2, seed=6, k=6, tag_size=sizes, depth=(1.2, 1.8))
    return g, sizes, {f"tag_{t}": float(sizes[t]) for t in range(8)}


def _detections(g, caps):
    for c in caps:
        sel = g.obs_cap == c
        yield f"cap{c}", [f"tag_{t}" for t in g.obs_tag[sel]], g.corners[sel]


@pytest.mark.parametrize("driver", ["solve", "solve_incremental"])
def test_slam_mirror_carries_the_sizes(lm, oracle, driver):
    g, sizes, by_id = _mirror_scene()
    s = lm.SlamSolver(elimination=lm.ELIM_CAPTURES)
    o = ref.sized_oracle_slam(oracle, by_id, camera=g.camera)
    s.set_camera(g.camera)
    for tid, v in by_id.items():
        s.set_aruco_size(tid, v)              # by id, before the first detection
    for uid, ids, corners in _detections(g, range(10)):
        s.add_detections(uid, ids, corners)
        o.add_detections(uid, ids, corners)
    getattr(s, driver)()
    getattr(o, driver)()
    assert [s.aruco_size(a) for a in range(s.num_arucos)] == [by_id[s.aruco(a)[0]] for a in range(s.num_arucos)]
    # the same flow as the CPU restatement of the drivers with the sized initialisers and the
    # dense LM (the tolerances of tests/test_gpu_slam.py: a chain of solves)
    assert s.num_solves == o.n_solves == 10 and s.solve_order() == o.solve_order
    last = s.last_summary()
    assert last["termination"] == o.last_summary["termination"]
    assert abs(last["final_cost"] - o.last_summary["final_cost"]) <= 1e-6 * o.last_summary["final_cost"]
    np.testing.assert_allclose(s.capture_poses()[:10], np.array([c["pose"] for c in o.captures]), atol=1e-5)
    np.testing.assert_allclose(s.aruco_poses(), np.array([a["pose"] for a in o.arucos]), atol=1e-5)
    assert synth.rms_px(last["final_cost"], int(np.sum(g.obs_cap < 10))) < 1.0
    # a pointer-keyed Problem of the same blocks and sizes from the values the last solve started at
    # in the CPU restatement (the mirror keeps no copy of its own; they agree to the 1e-5 above, and
    # the mirror's initialisers are pinned on their own in tests/test_tag_size.py)
    (camera, cap, tag, obs_cap, obs_tag, corners), tsz = o.last_start
    camera, caps, tags = camera.copy(), [c.copy() for c in cap], [t.copy() for t in tag]
    prob = lm.Problem(elimination=lm.ELIM_CAPTURES)
    for b in range(len(obs_cap)):
        prob.add_residual_block(corners[b], camera, caps[obs_cap[b]], tags[obs_tag[b]], size=tsz[obs_tag[b]])
    sp = prob.solve()
    print(f"{driver}: mirror final cost {last['final_cost']:.12e}, pointer-keyed {sp['final_cost']:.12e}")
    assert abs(sp["final_cost"] - last["final_cost"]) <= 1e-8 * last["final_cost"]
    # localize_many on the held-out captures: the Localizer on the mirror's map with the same sizes
    for uid, ids, corners in _detections(g, range(10, 12)):
        s.add_detections(uid, ids, corners)
    order = [s.aruco(a)[0] for a in range(s.num_arucos)]
    index = {tid: a for a, tid in enumerate(order)}
    sel = g.obs_cap >= 10
    batch = synth.LocalizeBatch(s.camera()[0].copy(), s.aruco_poses().copy(), np.array([0, 6, 12], np.int32),
                                np.array([index[f"tag_{t}"] for t in g.obs_tag[sel]], np.int32), g.corners[sel].copy(),
                                g.cap_true[10:12].copy(), np.ones(len(order), np.uint8))
    s.localize_many(10)
    pose, res, _ = lm.Localizer(batch, tag_size=[by_id[t] for t in order]).solve()
    assert (res["status"] == 0).all()
    np.testing.assert_array_equal(s.capture_poses()[10:12], pose)
    # metric: the two cameras are as far apart as in the truth (the map's gauge is the mirror's own)
    assert abs(np.linalg.norm(pose[0, :3] - pose[1, :3]) -
               np.linalg.norm(g.cap_true[10, :3] - g.cap_true[11, :3])) < 0.05


def test_slam_mirror_last_solve_from_its_own_initial_values(lm):
    """solveIncremental in two calls: nine captures, then the tenth.  The second call is one
    solveCapture, so the values its solve starts from are the mirror's state after the first call
    plus the mirror's own initialisers (arslam_slam_debug_init_pose, the same host code) on the new
    capture and on any tag it brings.  A pointer-keyed Problem of the same blocks (in the mirror's
    AddResidualBlock order), sides and those initial values ends at the mirror's final cost: 1e-8."""
    g, sizes, by_id = _mirror_scene()
    s = lm.SlamSolver(elimination=lm.ELIM_CAPTURES)
    s.set_camera(g.camera)
    for tid, v in by_id.items():
        s.set_aruco_size(tid, v)
    for uid, ids, corners in _detections(g, range(9)):
        s.add_detections(uid, ids, corners)
    s.solve_incremental()
    assert s.num_solves == 9
    camera = s.camera()[0].copy()
    caps = [p.copy() for p in s.capture_poses()]
    n_before = s.num_arucos
    tags = [p.copy() for p in s.aruco_poses()]
    known = [bool(s.aruco(a)[2]) for a in range(n_before)]
    order_before = s.solve_order()
    for uid, ids, corners in _detections(g, [9]):
        s.add_detections(uid, ids, corners)
    new_blocks = [b for b in range(s.num_blocks) if s.block(b)[0] == 9]
    # solveCapture(capture 9, its first block whose tag is initialised), restated with the mirror's initialisers
    tags += [np.zeros(6) for _ in range(s.num_arucos - n_before)]
    known += [False] * (s.num_arucos - n_before)
    init = next(b for b in new_blocks if known[s.block(b)[1]])
    a0 = s.block(init)[1]
    cap9 = lm.debug_slam_init_pose("capture", s.block(init)[2], camera, tags[a0], s.aruco_size(a0))
    for b in new_blocks:
        a = s.block(b)[1]
        if not known[a]:
            known[a] = True
            tags[a] = lm.debug_slam_init_pose("ar", s.block(b)[2], camera, cap9, s.aruco_size(a))
    caps.append(cap9)
    s.solve_incremental()
    assert s.num_solves == 10 and s.solve_order() == order_before + [9]
    last = s.last_summary()
    prob = lm.Problem(elimination=lm.ELIM_CAPTURES)
    cam = camera.copy()
    for c in s.solve_order():
        for b in [b for b in range(s.num_blocks) if s.block(b)[0] == c]:
            _, a, rect, added = s.block(b)
            assert added
            prob.add_residual_block(rect, cam, caps[c], tags[a], size=s.aruco_size(a))
    sp = prob.solve()
    print(f"mirror's last solve: initial cost {last['initial_cost']:.12e} / {sp['initial_cost']:.12e}, "
          f"final cost {last['final_cost']:.12e} / {sp['final_cost']:.12e}")
    assert abs(sp["initial_cost"] - last["initial_cost"]) <= 1e-12 * last["initial_cost"]
    assert abs(sp["final_cost"] - last["final_cost"]) <= 1e-8 * last["final_cost"]
    assert abs(len(sp["iterations"]) - len(last["iterations"])) <= 1 and sp["termination"] == last["termination"]
