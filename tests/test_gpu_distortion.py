"""GPU tests of the radial camera model (ARSLAM_CAMERA_RADIAL), against tests/distortion_ref.py.

The reference is the oracle's own chain rule under the model (distortion_ref's header), exact per
observation, so the tolerances are the project's own:
  * rows: those of tests/test_gpu_parity.py's test_residual_jacobian_matches_oracle (residual
    rtol 1e-12 / atol 1e-9, Jacobian 1e-12 of the row scale) on the draws of
    tests/test_gpu_tag_size.py (_random_obs: that test's draws where every corner has
    |p_z| / |p| >= 4.5e-3, the conditioning the bound holds for); two independent fp64
    evaluations of the radial rows agree to 4e-14 of the row scale on them;
  * LM traces: tag_size_ref.assert_same_trace, and the pose check after one rigid alignment;
  * pointer-keyed blocks against the SoA load: the same bits; appended blocks against a fresh
    load: 1e-9 per iteration cost, as tests/test_gpu_tag_size.py;
  * the forced multi-rank path against one rank: the bounds of its sized twin;
  * covariances: tol = 16 e_ref of the input, not below 1e-10 (tests/test_gpu_lm_cov.py);
  * the localizer: the bounds of tests/test_gpu_tag_size.py's sized localizer test.
Under ARSLAM_CAMERA_PINHOLE a camera that carries l1, l2 solves bit for bit as one with zeros.
"""
import functools

import numpy as np
import pytest

import distortion_ref as ref
import localize_ref
import tag_size_ref as tref
from ar_slam_amd import synth
from gauge import assert_poses_match
from loss_ref import CAUCHY
from tag_size_ref import arrays, assert_same_trace
from test_gpu_tag_size import _random_obs

pytestmark = pytest.mark.gpu

E_REF_CAP = 1e-9


# ---- 1. rows ----

def test_radial_rows_match_the_wrapper(lm, oracle):
    R = ref.RadialOracle(oracle)
    rng = np.random.default_rng(7)
    n = 512
    cam, cap, tag, corners, size = _random_obs(rng, n, [0.0635, 0.0635, 0.02, 0.30])
    ls = np.array([(0.0, 0.0), ref.STRONG, ref.MILD, (0.2, -0.05)])[np.arange(n) % 4]
    cam[:, 1:] = ls
    assert (np.sum(tag[:, 3:] ** 2, 1) == 0).sum() >= n // 8 and (np.sum(cap[:, 3:] ** 2, 1) < 1e-3).sum() >= n // 8
    sized = size != 0.0635
    assert sized.sum() >= n // 8 and (~sized).sum() >= n // 8
    r, J = lm.debug_residual_jacobian_model(cam, cap, tag, corners, lm.CAMERA_RADIAL, size)
    worst = 0.0
    for i in range(n):
        ro, Jo = tref.residual_jacobian(R, cam[i], cap[i], tag[i], corners[i], size[i])
        np.testing.assert_allclose(r[i], ro, rtol=1e-12, atol=1e-9)
        scale = np.abs(Jo).max(axis=1, keepdims=True) + 1e-300
        worst = max(worst, float(np.max(np.abs(J[i] - Jo) / scale)))
    print(f"radial rows: worst Jacobian error {worst:.2e} of the row scale")
    assert worst < 1e-12
    assert np.all(J[..., 1:3] == 0.0)                          # l1, l2 are held
    assert np.array_equal(J[..., 3:6], J[..., 9:12])
    # without sizes: the default side's instance gives the sized one's bits at 0.0635
    d = ~sized
    r0, J0 = lm.debug_residual_jacobian_model(cam[d], cap[d], tag[d], corners[d], lm.CAMERA_RADIAL)
    assert np.array_equal(r0, r[d]) and np.array_equal(J0, J[d])
    # under PINHOLE the entry is debug_residual_jacobian, whatever l1, l2 the camera carries
    rp, Jp = lm.debug_residual_jacobian_model(cam, cap, tag, corners, lm.CAMERA_PINHOLE)
    rq, Jq = lm.debug_residual_jacobian(cam, cap, tag, corners)
    assert np.array_equal(rp, rq) and np.array_equal(Jp, Jq)


# ---- 2. the default is untouched ----

def _trace(s):
    return [(it["cost"], it["gradient_max_norm"], it["step_norm"], it["trust_region_radius"]) for it in s["iterations"]]


@pytest.mark.parametrize("loss", [None, (CAUCHY, 3.0)], ids=["plain", "cauchy"])
def test_pinhole_ignores_l1_l2_bit_for_bit(lm, loss):
    g = tref.trace_graphs()["gk11"][0]   # (the one-chunk and the chunked instances; pinhole detections)
    a = lm.ResidentProblem(*arrays(g), loss=loss)
    b = lm.ResidentProblem(*ref.with_distortion(arrays(g), ref.MILD), loss=loss)
    sa, sb = a.solve(), b.solve()
    assert _trace(sb) == _trace(sa)
    assert sb["final_cost"] == sa["final_cost"] and b.camera[0] == a.camera[0]
    assert np.array_equal(b.camera[1:], ref.MILD)          # held, and handed back
    assert np.array_equal(b.cap, a.cap) and np.array_equal(b.tag, a.tag)


LOC_FIELDS = ["status", "rule", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "init_obs",
              "initial_cost", "final_cost"]


def test_pinhole_localizer_ignores_l1_l2_bit_for_bit(lm):
    import dataclasses
    b = synth.make_localize_batch(map_name="medium", n_query=96)
    cam = b.camera.copy()
    cam[1:] = ref.MILD
    p0, r0, _ = lm.Localizer(b).solve()
    p1, r1, _ = lm.Localizer(dataclasses.replace(b, camera=cam)).solve()
    assert np.array_equal(p1, p0)
    for f in LOC_FIELDS:
        np.testing.assert_array_equal(r1[f], r0[f], err_msg=f)


# ---- 3. traces against the dense LM ----

def _losses(g, with_loss):
    if not with_loss:
        return None
    return np.full(g.n_obs, CAUCHY, np.uint8), np.full(g.n_obs, 3.0)


@functools.lru_cache(maxsize=None)
def _dense(oracle, name, with_loss, sized=False):
    g, camc, capc, tagc, sizes = ref.trace_graphs(ref.MILD, sized)[name]
    kinds, a = (CAUCHY, 3.0) if with_loss else (0, 0.0)
    return tref.solve(ref.RadialOracle(oracle), arrays(g), sizes, camc, capc, tagc, kinds, a)


def _check_trace(lm, oracle, name, with_loss, sized=False, **opts):
    g, camc, capc, tagc, sizes = ref.trace_graphs(ref.MILD, sized)[name]
    want = _dense(oracle, name, with_loss, sized)
    rp = lm.ResidentProblem(*arrays(g), camc, capc, tagc, obs_loss=_losses(g, with_loss), tag_size=sizes,
                            camera_model=lm.CAMERA_RADIAL, **opts)
    s = rp.solve()
    ours = (rp.camera, rp.cap, rp.tag, s)
    assert_same_trace(ours, want)
    assert_poses_match(ours[1], ours[2], want[1], want[2], tags=np.unique(g.obs_tag), caps=np.unique(g.obs_cap))
    assert s["termination"] == "CONVERGENCE"
    assert np.array_equal(rp.camera[1:], ref.MILD)         # held
    return s


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
@pytest.mark.parametrize("name", ["g6", "g20", "gk11", "g20_tag_const", "g20_cap_const", "g20_camera_const"])
def test_radial_trace_matches_the_dense_lm(lm, oracle, name, with_loss):
    _check_trace(lm, oracle, name, with_loss)


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
@pytest.mark.parametrize("side", ["ELIM_CAPTURES", "ELIM_TAGS", "ELIM_MIXED"])
def test_radial_trace_under_every_elimination(lm, oracle, side, with_loss):
    s = _check_trace(lm, oracle, "g20", with_loss, elimination=getattr(lm, side))
    assert s["elimination_used"] in (getattr(lm, side), lm.ELIM_CAPTURES, lm.ELIM_TAGS)
    if side != "ELIM_MIXED":
        assert s["elimination_used"] == getattr(lm, side)


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
def test_radial_trace_with_mixed_tag_sides(lm, oracle, with_loss):
    """The kSized x kDist instances: one side per tag, detections of tags of those sides through the lens."""
    sizes = ref.trace_graphs(ref.MILD, True)["g20"][4]
    assert len(np.unique(sizes)) > 1
    _check_trace(lm, oracle, "g20", with_loss, sized=True)


# ---- 4. paths ----

def _add(prob, g, camera, caps, tags, blocks):
    for b in blocks:
        prob.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]])


def test_pointer_keyed_blocks_equal_the_soa_load(lm):
    """The pointer-keyed handle numbers its blocks in the order it first sees them; the SoA load of
    the same problem in that numbering is the same load, so the same bits."""
    g = ref.trace_graphs(ref.MILD)["g20"][0]
    camera, caps, tags = g.camera.copy(), [c.copy() for c in g.cap], [t.copy() for t in g.tag]
    prob = lm.Problem()
    prob.set_camera_model(lm.CAMERA_RADIAL)
    _add(prob, g, camera, caps, tags, range(g.n_obs))
    s = prob.solve()
    _, first = np.unique(g.obs_tag, return_index=True)
    order = g.obs_tag[np.sort(first)]                      # tags as first seen
    assert len(order) == g.n_tag and np.array_equal(np.unique(g.obs_cap), np.arange(g.n_cap))
    rank = np.empty(g.n_tag, np.int32)
    rank[order] = np.arange(g.n_tag, dtype=np.int32)
    rp = lm.ResidentProblem(g.camera, g.cap, g.tag[order], g.obs_cap, rank[g.obs_tag], g.corners,
                            camera_model=lm.CAMERA_RADIAL)
    s2 = rp.solve()
    assert _trace(s) == _trace(s2)
    assert np.array_equal(camera, rp.camera) and np.array_equal(np.array(caps), rp.cap)
    assert np.array_equal(np.array(tags)[order], rp.tag)
    # and the model took part: the same blocks as a pinhole start from another cost
    pin = lm.ResidentProblem(*arrays(g)).solve()
    assert abs(pin["initial_cost"] - s2["initial_cost"]) > 1e-3 * s2["initial_cost"]


def test_appended_blocks_keep_the_plan_and_equal_a_fresh_load(lm):
    g = ref.trace_graphs(ref.MILD)["g20"][0]
    # captures whose tags and tag pairs the first 14 already have (a fourth, 19, would be a quarter
    # more groups than the order was made for, and the handle then reloads with a fresh order)
    first, added = 14, [14, 15, 17]
    camera, caps, tags = g.camera.copy(), [c.copy() for c in g.cap], [t.copy() for t in g.tag]
    prob = lm.Problem(elimination=lm.ELIM_CAPTURES)
    prob.set_camera_model(lm.CAMERA_RADIAL)
    _add(prob, g, camera, caps, tags, np.nonzero(g.obs_cap < first)[0])
    s1 = prob.solve()
    assert s1["setup_kind"] == lm.SETUP_LOAD
    for c in added:
        _add(prob, g, camera, caps, tags, np.nonzero(g.obs_cap == c)[0])
    start = (camera.copy(), [c.copy() for c in caps], [t.copy() for t in tags])
    s2 = prob.solve()
    assert s2["setup_kind"] == lm.SETUP_APPEND, s2["setup_kind"]
    fresh = lm.Problem(elimination=lm.ELIM_CAPTURES)
    fresh.set_camera_model(lm.CAMERA_RADIAL)
    cam_f, caps_f, tags_f = start[0].copy(), [c.copy() for c in start[1]], [t.copy() for t in start[2]]
    _add(fresh, g, cam_f, caps_f, tags_f, np.nonzero(g.obs_cap < first)[0])
    for c in added:
        _add(fresh, g, cam_f, caps_f, tags_f, np.nonzero(g.obs_cap == c)[0])
    s3 = fresh.solve()
    assert s3["setup_kind"] == lm.SETUP_LOAD
    assert [i["step_is_successful"] for i in s2["iterations"]] == [i["step_is_successful"] for i in s3["iterations"]]
    for a, b in zip(s2["iterations"], s3["iterations"]):
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"]
    assert abs(camera[0] - cam_f[0]) <= 1e-8 * cam_f[0]
    # the appended problem kept the model: as a pinhole the same blocks start from another cost
    plain = lm.Problem(elimination=lm.ELIM_CAPTURES)
    cam_p, caps_p, tags_p = start[0].copy(), [c.copy() for c in start[1]], [t.copy() for t in start[2]]
    _add(plain, g, cam_p, caps_p, tags_p, np.nonzero(g.obs_cap < first)[0])
    for c in added:
        _add(plain, g, cam_p, caps_p, tags_p, np.nonzero(g.obs_cap == c)[0])
    assert abs(plain.solve()["initial_cost"] - s2["initial_cost"]) > 1e-3 * s2["initial_cost"]


def test_forced_multirank_path_carries_the_model(lm):
    g = ref.trace_graphs(ref.MILD)["g20"][0]
    plain = lm.ResidentProblem(*arrays(g), camera_model=lm.CAMERA_RADIAL)
    sp = plain.solve()
    multi = lm.ResidentProblem(*arrays(g), camera_model=lm.CAMERA_RADIAL, comm=(0, 1, lambda a, op: None),
                               force_multirank=True)
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


def test_set_camera_model_drops_a_loaded_problem(lm, oracle):
    g = ref.trace_graphs(ref.MILD)["g6"][0]
    rp = lm.ResidentProblem(*arrays(g))
    s0 = rp.solve()
    rp.set_camera_model(lm.CAMERA_PINHOLE)      # (the model it has: the problem stays)
    assert rp.solve()["initial_cost"] == s0["initial_cost"]
    rp.set_camera_model(lm.CAMERA_RADIAL)
    with pytest.raises(lm.LMError) as e:
        rp.solve()
    assert e.value.code == -7   # ARSLAM_E_STATE: nothing loaded
    with pytest.raises(lm.LMError) as e:
        rp.covariance()
    assert e.value.code == -7
    # a later load uses it
    u = lm.ResidentProblem(*arrays(g), camera_model=lm.CAMERA_RADIAL)
    want = tref.terms(ref.RadialOracle(oracle), arrays(g), None).cost
    su = u.solve()
    assert abs(su["initial_cost"] - want) <= 1e-9 * want
    assert abs(s0["initial_cost"] - want) > 1e-3 * want


# ---- 5. the scene of the README ----

def test_scene_device_against_the_dense_lm(lm, oracle):
    g = ref.scene()
    A = arrays(g)
    want = tref.solve(ref.RadialOracle(oracle), A)
    rp = lm.ResidentProblem(*A, camera_model=lm.CAMERA_RADIAL)
    s = rp.solve()
    radial = (rp.camera, rp.cap, rp.tag, s)
    assert_same_trace(radial, want)
    pp = lm.ResidentProblem(*A)
    pinhole = (pp.camera, pp.cap, pp.tag, pp.solve())
    rms_r, rms_p, f_r, f_p = ref.scene_figures(g, radial, pinhole)
    print(f"scene l = {ref.SCENE} on the device: with the model RMS {rms_r:.3f} px, f = {f_r:.1f}; as a pinhole "
          f"RMS {rms_p:.3f} px, f = {f_p:.1f} (truth 900); dense LM with the model f = {want[0][0]:.1f}")
    ref.assert_scene(rms_r, rms_p, f_r, f_p)


# ---- 6. the localizer ----

def _rot_err(w1, w2):
    R1, R2 = synth.rodrigues(w1), synth.rodrigues(w2)
    return np.arccos(np.clip((np.einsum("nij,nij->n", R1, R2) - 1.0) / 2.0, -1.0, 1.0))


@pytest.fixture(scope="module")
def radial96():
    """96 queries against the 80-tag map of "medium" through the MILD lens, and the same with one
    detection per query shifted 40 px."""
    b = synth.make_localize_batch(map_name="medium", n_query=96, distortion=ref.MILD)
    b.tag_in_map = np.ones(b.tag.shape[0], np.uint8)
    b.tag_in_map[b.obs_tag[b.q_start[9]]] = 0    # query 9 initialises from a later block
    return b, localize_ref.shifted_batch(b, seed=11, px=40.0)[0]


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
@pytest.mark.parametrize("init_from_map", [1, 0])
def test_radial_localizer_matches_numpy(lm, oracle, radial96, init_from_map, with_loss):
    R = ref.RadialOracle(oracle)
    clean, shifted = radial96
    b = shifted if with_loss else clean
    kinds, scales = ((CAUCHY, 3.0) if with_loss else (None, None))
    loss = (CAUCHY, 3.0) if with_loss else None
    pose0 = None if init_from_map else b.pose_true + 0.01
    want = tref.localize(R, b, tref.DEFAULT, kinds, scales, init_from_map=bool(init_from_map), pose=pose0)
    loc = lm.Localizer(b, init_from_map=bool(init_from_map), pose=pose0, loss=loss, camera_model=lm.CAMERA_RADIAL)
    assert loc.camera_model() == lm.CAMERA_RADIAL
    pose, res, _ = loc.solve()
    assert (want["status"] == 0).all()           # every query converges in the reference
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
    # observation_terms and covariance on the same batch, at the device's poses
    s, w = loc.observation_terms()
    so = tref.MapSizedOracle(R, b.tag, tref.DEFAULT)
    s_ref, w_ref = localize_ref.observation_terms(so, b, pose, kinds, scales, res["status"])
    np.testing.assert_allclose(s, s_ref, rtol=1e-12)
    np.testing.assert_allclose(w, w_ref, rtol=1e-12)
    cov, st, mp = loc.covariance()
    c_ref, s_st, m_ref = tref.localize_covariance(R, b, tref.DEFAULT, pose, kinds, scales, res["status"], res["rule"])
    np.testing.assert_array_equal(st, s_st)
    assert (m_ref >= 1e-4).all(), m_ref.min()      # the 1e-9 below rests on this (tests/test_gpu_localize_cov.py)
    d = np.sqrt(np.einsum("qii->qi", c_ref))
    err = (np.abs(cov - c_ref) / (d[:, :, None] * d[:, None, :])).max()
    print(f"covariance {err:.2e} relative to sqrt(C_ii C_jj), min_pivot {np.abs(mp - m_ref).max():.2e} absolute")
    assert err <= 1e-9
    assert np.abs(mp - m_ref).max() <= 1e-12
    np.testing.assert_array_equal(cov, cov.transpose(0, 2, 1))
    # the same queries solved as a pinhole, all the localizer could do before: the map is fixed and
    # cannot absorb the lens, so the pose takes it
    pin = lm.Localizer(b, init_from_map=bool(init_from_map), pose=pose0, loss=loss)
    pose_p, _, _ = pin.solve()
    e_r = np.linalg.norm(pose[:, :3] - b.pose_true[:, :3], axis=1)
    e_p = np.linalg.norm(pose_p[:, :3] - b.pose_true[:, :3], axis=1)
    print(f"median translation error of 96 queries: {1e3 * np.median(e_r):.2f} mm with the model, "
          f"{1e3 * np.median(e_p):.2f} mm as a pinhole")
    assert np.median(e_r) < np.median(e_p)
    # a change of model asks for a new solve before the terms or the covariance
    loc.set_camera_model(lm.CAMERA_PINHOLE)
    with pytest.raises(lm.LMError) as e:
        loc.covariance()
    assert e.value.code == -7
    pose_q, _, _ = loc.solve()
    assert np.array_equal(pose_q, pose_p)


# ---- 7. covariance ----

@pytest.mark.parametrize("side", ["ELIM_CAPTURES", "ELIM_TAGS"])
def test_covariance_under_the_model(lm, oracle, side):
    R = ref.RadialOracle(oracle)
    g = ref.trace_graphs(ref.MILD)["g20"][0]
    elimination = getattr(lm, side)
    tc = np.zeros(g.n_tag, np.uint8)
    tc[0] = 1
    rp = lm.ResidentProblem(*arrays(g), tag_const=tc, camera_model=lm.CAMERA_RADIAL, elimination=elimination)
    s = rp.solve()
    assert s["elimination_used"] == elimination
    out = rp.covariance()
    at = (rp.camera, rp.cap, rp.tag, g.obs_cap, g.obs_tag, g.corners)
    want = tref.covariance(R, at, None, tag_const=tc, scale_arrays=arrays(g))
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
    T, Cp, Cm = lm.BLOCK_TAG, lm.BLOCK_CAPTURE, lm.BLOCK_CAMERA
    pairs = [((T, 1), (T, g.n_tag - 1)), ((T, 2), (T, 3)), ((Cp, 0), (T, 5)), ((T, 5), (Cp, 0)), ((Cp, 1), (Cp, 7)),
             ((Cm, 0), (T, 4)), ((Cp, 2), (Cm, 0)), ((T, 6), (T, 6)), ((T, 0), (T, 1))]
    cov, st, _ = rp.covariance_pairs(pairs)
    pw = tref.covariance_pairs(R, at, None, pairs, tag_const=tc, scale_arrays=arrays(g))
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


# ---- 8. the SLAM mirror ----

def _detections(g, caps):
    for c in caps:
        sel = g.obs_cap == c
        yield f"cap{c}", [f"tag_{t}" for t in g.obs_tag[sel]], g.corners[sel]


@pytest.mark.parametrize("driver", ["solve", "solve_incremental"])
def test_slam_mirror_carries_the_model(lm, oracle, driver, tmp_path):
    """The scene of tests/test_gpu_tag_size.py's mirror test -- 10 captures of an 8-tag wall
    (4 x 2), 6 tags each, one side per tag -- through the MILD lens; the initialisers are the
    pinhole's on both sides (they only seed the LM).  With every tag at 0.0635 m the same wall is
    so weakly conditioned from 1.2 to 1.8 m that the dense reference's own chain runs several
    solves to the iteration limit, with or without a lens, and a chain of unconverged solves
    compares nothing; on this scene every solve of the reference converges in at most 18
    iterations."""
    R = ref.RadialOracle(oracle)
    sizes = tref.tag_sizes(8, seed=4)
    by_id = {f"tag_{t}": float(sizes[t]) for t in range(8)}
    g = synth.make_graph(12, 4, 2, seed=6, k=6, tag_size=sizes, depth=(1.2, 1.8), distortion=ref.MILD)
    s = lm.SlamSolver(elimination=lm.ELIM_CAPTURES)
    o = tref.sized_oracle_slam(R, by_id, camera=g.camera)
    s.set_camera(g.camera)
    s.set_camera_model(lm.CAMERA_RADIAL)
    for tid, v in by_id.items():
        s.set_aruco_size(tid, v)
    for uid, ids, corners in _detections(g, range(10)):
        s.add_detections(uid, ids, corners)
        o.add_detections(uid, ids, corners)
    getattr(s, driver)()
    getattr(o, driver)()
    with pytest.raises(lm.LMError) as e:
        s.set_camera_model(lm.CAMERA_PINHOLE)      # residual blocks exist: the model is bound
    assert e.value.code == -7
    assert s.num_solves == o.n_solves == 10 and s.solve_order() == o.solve_order
    last = s.last_summary()
    assert last["termination"] == o.last_summary["termination"]
    assert abs(last["final_cost"] - o.last_summary["final_cost"]) <= 1e-6 * o.last_summary["final_cost"]
    np.testing.assert_allclose(s.capture_poses()[:10], np.array([c["pose"] for c in o.captures]), atol=1e-5)
    np.testing.assert_allclose(s.aruco_poses(), np.array([a["pose"] for a in o.arucos]), atol=1e-5)
    assert synth.rms_px(last["final_cost"], int(np.sum(g.obs_cap < 10))) < 1.0
    assert np.array_equal(s.camera()[0][1:], ref.MILD)
    assert np.array_equal(s.camera_distortion(), [*ref.MILD, 0.0, 0.0, 0.0])
    # a pointer-keyed Problem of the same blocks under the model, from the values the last solve
    # started at in the CPU restatement (as tests/test_gpu_tag_size.py's mirror test)
    (camera, cap, tag, obs_cap, obs_tag, corners), tsz = o.last_start
    camera, caps, tags = camera.copy(), [c.copy() for c in cap], [t.copy() for t in tag]
    prob = lm.Problem(elimination=lm.ELIM_CAPTURES)
    prob.set_camera_model(lm.CAMERA_RADIAL)
    for b in range(len(obs_cap)):
        prob.add_residual_block(corners[b], camera, caps[obs_cap[b]], tags[obs_tag[b]], size=tsz[obs_tag[b]])
    sp = prob.solve()
    print(f"{driver}: mirror final cost {last['final_cost']:.12e}, pointer-keyed {sp['final_cost']:.12e}")
    assert abs(sp["final_cost"] - last["final_cost"]) <= 1e-8 * last["final_cost"]
    # localize_many on the held-out captures: the Localizer on the mirror's map under the model
    for uid, ids, corners in _detections(g, range(10, 12)):
        s.add_detections(uid, ids, corners)
    order = [s.aruco(a)[0] for a in range(s.num_arucos)]
    index = {tid: a for a, tid in enumerate(order)}
    sel = g.obs_cap >= 10
    batch = synth.LocalizeBatch(s.camera()[0].copy(), s.aruco_poses().copy(), np.array([0, 6, 12], np.int32),
                                np.array([index[f"tag_{t}"] for t in g.obs_tag[sel]], np.int32), g.corners[sel].copy(),
                                g.cap_true[10:12].copy(), np.ones(len(order), np.uint8))
    s.localize_many(10)
    tsz = [by_id[t] for t in order]
    pose, res, _ = lm.Localizer(batch, tag_size=tsz, camera_model=lm.CAMERA_RADIAL).solve()
    assert (res["status"] == 0).all()
    np.testing.assert_array_equal(s.capture_poses()[10:12], pose)
    pose_p, _, _ = lm.Localizer(batch, tag_size=tsz).solve()
    assert not np.array_equal(pose_p, pose)
    # map -> save -> load -> the same model
    s.save_yaml(tmp_path / "m.yaml")
    t = lm.SlamSolver()
    t.load_yaml(tmp_path / "m.yaml")
    assert t.camera_model() == lm.CAMERA_RADIAL
    assert np.array_equal(t.camera_distortion(), s.camera_distortion())
    np.testing.assert_array_equal(t.aruco_poses(), s.aruco_poses())
