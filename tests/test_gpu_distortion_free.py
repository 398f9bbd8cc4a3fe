"""GPU tests of the estimated distortion (arslam_lm_set_estimate_distortion), against
tests/distortion_free_ref.py.  Inputs: distortion_ref.trace_graphs(MILD) -- detections through the
lens (-0.12, 0.03) -- with the camera's l1, l2 set to zero before the solve.

  * rows: the two l columns against the helper at the bound of tests/test_gpu_distortion.py's row
    test, 1e-12 of the row scale, on its draws.
  * border: reduced rows cam_row + 1, cam_row + 2 of the assembled system (the debug entry: the
    linearization, k_schur, the gathers and k_schur_cam with its gather, no factorization) against
    the dense normal matrix Js'Js + D^2 reduced in numpy long double, e(row) = max_j |delta| /
    sqrt(S_ii S_jj) over the reduced columns and the right-hand side (whose S_jj is the reduced
    r'r).  Row cam_row is the code every problem runs, on the same input: the two new rows must
    satisfy e <= 8 max(e(cam_row), 2.3e-16) -- the 8 for another summation order over at most 11
    observations, 2.3e-16 one rounding.
  * traces: tag_size_ref.solve on the helper with tag_size_ref.assert_same_trace, and
    |delta l1|, |delta l2| <= 1e-8 (the reference's own f64 and long-double solves differ by
    <= 5e-14 there: far above rounding, far below any real difference).
  * the README's scene from l = 0: the CPU test's three assertions, and the dense reference's RMS
    to 1e-8 relative.
  * off is off, determinism: bit for bit.  Refusals: ARSLAM_E_UNSUPPORTED, the handle still usable.
"""
import functools

import numpy as np
import pytest

import distortion_free_ref as fref
import distortion_ref as ref
import tag_size_ref as tref
from ar_slam_amd import synth
from loss_ref import CAUCHY
from tag_size_ref import arrays, assert_same_trace
from test_gpu_tag_size import _random_obs

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2
L_TOL = 1e-8


def _losses(g, with_loss):
    if not with_loss:
        return None
    return np.full(g.n_obs, CAUCHY, np.uint8), np.full(g.n_obs, 3.0)


def _trace(s):
    return [(it["cost"], it["gradient_max_norm"], it["step_norm"], it["trust_region_radius"]) for it in s["iterations"]]


# ---- 1. rows ----

def test_l_columns_match_the_helper(lm, oracle):
    R = fref.FreeRadialOracle(oracle)
    rng = np.random.default_rng(7)
    n = 512
    cam, cap, tag, corners, size = _random_obs(rng, n, [0.0635, 0.0635, 0.02, 0.30])
    cam[:, 1:] = np.array([(0.0, 0.0), ref.STRONG, ref.MILD, (0.2, -0.05)])[np.arange(n) % 4]
    r, Jl = lm.debug_residual_jacobian_distortion(cam, cap, tag, corners, size)
    rh, Jh = lm.debug_residual_jacobian_model(cam, cap, tag, corners, lm.CAMERA_RADIAL, size)
    assert np.array_equal(r, rh)                       # the residual is the held model's
    worst = 0.0
    for i in range(n):
        _, Jo = tref.residual_jacobian(R, cam[i], cap[i], tag[i], corners[i], size[i])
        scale = np.abs(Jo).max(axis=1, keepdims=True) + 1e-300
        worst = max(worst, float(np.max(np.abs(Jl[i] - Jo[:, 1:3]) / scale)))
    print(f"l columns: worst error {worst:.2e} of the row scale")
    assert worst < 1e-12
    d = size == 0.0635                                 # the default side's instance: the sized one's bits
    r0, Jl0 = lm.debug_residual_jacobian_distortion(cam[d], cap[d], tag[d], corners[d])
    assert np.array_equal(r0, r[d]) and np.array_equal(Jl0, Jl[d])


# ---- 2. the border of the Schur complement ----

def _ld_spd_solve(A, B):
    """A^-1 B in numpy long double, A SPD (a column Cholesky and two triangular solves)."""
    n = len(A)
    Lc = np.array(A, np.longdouble)
    for j in range(n):
        Lc[j, j] = np.sqrt(Lc[j, j] - Lc[j, :j] @ Lc[j, :j])
        if j + 1 < n:
            Lc[j + 1:, j] = (Lc[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
    Y = np.array(B, np.longdouble)
    for j in range(n):
        Y[j] = (Y[j] - Lc[j, :j] @ Y[:j]) / Lc[j, j]
    for j in range(n - 1, -1, -1):
        Y[j] = (Y[j] - Lc[j + 1:, j] @ Y[j + 1:]) / Lc[j, j]
    return Y


@functools.lru_cache(maxsize=None)
def _dense_reduced(oracle, name, with_loss, tags_eliminated, radius):
    """The reduced system of the problem at its start, in long double: (S over the f-side slots,
    rhs, reduced r'r, the f-side slots), the e-side the captures or the tags."""
    g = ref.trace_graphs(ref.MILD)[name][0]
    kinds, a = (CAUCHY, 3.0) if with_loss else (0, 0.0)
    P = tref._Problem(fref.FreeRadialOracle(oracle), fref.zero_lens(arrays(g)), None, False, None, None, kinds, a)
    _, J, r, ok = P.linearize(P.x0)
    assert ok and P.free.all()
    colnorm = np.sum(J * J, axis=0)
    scale = 1.0 / (1.0 + np.sqrt(colnorm))
    diag = np.clip(scale * scale * colnorm, tref.OPTIONS["min_lm_diagonal"], tref.OPTIONS["max_lm_diagonal"])
    dk = np.sqrt(diag / radius)
    Js = np.array(J, np.longdouble) * np.array(scale, np.longdouble)
    rl = np.array(r, np.longdouble)
    H = Js.T @ Js + np.diag(np.array(dk * dk, np.longdouble))
    b = Js.T @ rl
    cap_slots, tag_slots = np.arange(3, 3 + 6 * P.nc), np.arange(3 + 6 * P.nc, P.n)
    e = tag_slots if tags_eliminated else cap_slots
    f = np.concatenate([np.arange(3), cap_slots if tags_eliminated else tag_slots])
    X = _ld_spd_solve(H[np.ix_(e, e)], np.concatenate([H[np.ix_(e, f)], b[e, None]], axis=1))
    S = H[np.ix_(f, f)] - H[np.ix_(f, e)] @ X[:, :-1]
    rhs = b[f] - H[np.ix_(f, e)] @ X[:, -1]
    rr = rl @ rl - b[e] @ X[:, -1]
    return S, rhs, rr, f


@pytest.mark.parametrize("side", ["ELIM_CAPTURES", "ELIM_TAGS"])
@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
@pytest.mark.parametrize("name", ["g6", "g20", "gk11"])
def test_border_rows_match_the_dense_reduction(lm, oracle, name, with_loss, side):
    g = ref.trace_graphs(ref.MILD)[name][0]
    if name == "gk11":   # captures of 11 observations (the chunked rows) and of more than 10 distinct tags
        per_cap = [len(np.unique(g.obs_tag[g.obs_cap == c])) for c in range(g.n_cap)]
        assert np.bincount(g.obs_cap).max() >= 11 and max(per_cap) > 10
    radius = 1e4
    tags_e = side == "ELIM_TAGS"
    rp = lm.ResidentProblem(*fref.zero_lens(arrays(g)), obs_loss=_losses(g, with_loss), camera_model=lm.CAMERA_RADIAL,
                            estimate_distortion=True, elimination=getattr(lm, side))
    rows, slot = rp.debug_camera_rows(radius)
    cap_row, tag_row, cam_row = rp.debug_reduced_rows()
    assert list(slot) == [0, 1, 2] and cam_row >= 0
    S, rhs, rr, f = _dense_reduced(oracle, name, with_loss, tags_e, radius)
    # the reduced row of each f-side slot of the reference
    blk_row = cap_row if tags_e else tag_row
    n_blk = len(blk_row)
    assert np.all(blk_row >= 0) and len(f) == 3 + 6 * n_blk
    row_of = np.concatenate([cam_row + np.arange(3), (blk_row[:, None] + np.arange(6)[None, :]).reshape(-1)])
    n_red = cam_row + 3
    assert rows.shape == (3, n_red + 1)
    padding = np.setdiff1d(np.arange(n_red), row_of)
    assert np.all(rows[:, padding] == 0.0)
    d = np.sqrt(np.array(np.diag(S), np.float64))
    e = []
    for b in range(3):
        dm = np.abs(rows[b, row_of] - np.array(S[b], np.float64)) / (d[b] * d)
        dr = abs(rows[b, n_red] - float(rhs[b])) / (d[b] * np.sqrt(float(rr)))
        e.append(max(float(dm.max()), float(dr)))
    print(f"border {name} {'cauchy' if with_loss else 'plain'} {side}: e(f) = {e[0]:.2e}, e(l1) = {e[1]:.2e}, e(l2) = {e[2]:.2e}")
    assert np.abs(rows[1:, row_of]).max() > 0.0
    bound = 8.0 * max(e[0], 2.3e-16)
    assert e[1] <= bound and e[2] <= bound


# ---- 3. traces against the dense LM ----

@functools.lru_cache(maxsize=None)
def _dense(oracle, name, with_loss, sized=False):
    g, camc, capc, tagc, sizes = ref.trace_graphs(ref.MILD, sized)[name]
    kinds, a = (CAUCHY, 3.0) if with_loss else (0, 0.0)
    return tref.solve(fref.FreeRadialOracle(oracle), fref.zero_lens(arrays(g)), sizes, camc, capc, tagc, kinds, a)


def _assert_same(ours, want):
    assert_same_trace(ours, want)
    assert abs(ours[0][1] - want[0][1]) <= L_TOL and abs(ours[0][2] - want[0][2]) <= L_TOL, (ours[0], want[0])


def _check_trace(lm, oracle, name, with_loss, sized=False, **opts):
    g, camc, capc, tagc, sizes = ref.trace_graphs(ref.MILD, sized)[name]
    want = _dense(oracle, name, with_loss, sized)
    A = fref.zero_lens(arrays(g))
    rp = lm.ResidentProblem(*A, camc, capc, tagc, obs_loss=_losses(g, with_loss), tag_size=sizes,
                            camera_model=lm.CAMERA_RADIAL, estimate_distortion=True, **opts)
    s = rp.solve()
    _assert_same((rp.camera, rp.cap, rp.tag, s), want)
    assert s["termination"] == "CONVERGENCE"
    if camc:
        assert np.array_equal(rp.camera, A[0])              # a constant camera block holds all three, bit for bit
    else:
        assert abs(rp.camera[1]) > 1e-3                     # and a free one moved off the start
    return rp, s


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
@pytest.mark.parametrize("name", ["g6", "g20", "gk11", "g20_tag_const", "g20_cap_const", "g20_camera_const"])
def test_trace_matches_the_dense_lm(lm, oracle, name, with_loss):
    _check_trace(lm, oracle, name, with_loss)


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
@pytest.mark.parametrize("side", ["ELIM_CAPTURES", "ELIM_TAGS", "ELIM_AUTO"])
@pytest.mark.parametrize("name", ["g20", "gk11"])
def test_trace_under_the_eliminations(lm, oracle, name, side, with_loss):
    _, s = _check_trace(lm, oracle, name, with_loss, elimination=getattr(lm, side))
    if side != "ELIM_AUTO":
        assert s["elimination_used"] == getattr(lm, side)


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
def test_trace_with_mixed_tag_sides(lm, oracle, with_loss):
    sizes = ref.trace_graphs(ref.MILD, True)["g20"][4]
    assert len(np.unique(sizes)) > 1
    _check_trace(lm, oracle, "g20", with_loss, sized=True)


@pytest.mark.parametrize("executor", [0, 1])
def test_trace_on_both_factor_executors(lm, oracle, executor):
    _check_trace(lm, oracle, "g20", False, factor_executor=executor)


def _pointer_keyed(lm, g, with_loss):
    camera = fref.zero_lens(arrays(g))[0].copy()
    caps, tags = [c.copy() for c in g.cap], [t.copy() for t in g.tag]
    prob = lm.Problem()
    prob.set_camera_model(lm.CAMERA_RADIAL)
    prob.set_estimate_distortion(True)
    for b in range(g.n_obs):
        prob.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]],
                                loss=(CAUCHY, 3.0) if with_loss else None)
    return prob, camera, caps, tags


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
def test_pointer_keyed_path_and_a_values_only_second_solve(lm, oracle, with_loss):
    g = ref.trace_graphs(ref.MILD)["g20"][0]
    want = _dense(oracle, "g20", with_loss)
    prob, camera, caps, tags = _pointer_keyed(lm, g, with_loss)
    start = (camera.copy(), [c.copy() for c in caps], [t.copy() for t in tags])
    s1 = prob.solve()
    assert s1["setup_kind"] == lm.SETUP_LOAD
    _assert_same((camera, np.array(caps), np.array(tags), s1), want)
    end = (camera.copy(), np.array(caps), np.array(tags))
    # the same structure again from the same start: a values-only reload, and the same bits
    camera[:] = start[0]
    for c, c0 in zip(caps, start[1]):
        c[:] = c0
    for t, t0 in zip(tags, start[2]):
        t[:] = t0
    s2 = prob.solve()
    assert s2["setup_kind"] == lm.SETUP_VALUES
    assert _trace(s2) == _trace(s1)
    assert np.array_equal(camera, end[0]) and np.array_equal(np.array(caps), end[1]) and np.array_equal(np.array(tags), end[2])


def test_appended_blocks_load_in_full_and_equal_a_fresh_load(lm):
    g = ref.trace_graphs(ref.MILD)["g20"][0]
    first, added = 14, [14, 15, 17]
    cam0 = fref.zero_lens(arrays(g))[0]

    def build(blocks_then):
        camera, caps, tags = cam0.copy(), [c.copy() for c in g.cap], [t.copy() for t in g.tag]
        prob = lm.Problem(elimination=lm.ELIM_CAPTURES)
        prob.set_camera_model(lm.CAMERA_RADIAL)
        prob.set_estimate_distortion(True)
        for b in np.nonzero(g.obs_cap < first)[0]:
            prob.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]])
        return prob, camera, caps, tags

    prob, camera, caps, tags = build(None)
    assert prob.solve()["setup_kind"] == lm.SETUP_LOAD
    for c in added:
        for b in np.nonzero(g.obs_cap == c)[0]:
            prob.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]])
    start = (camera.copy(), [c.copy() for c in caps], [t.copy() for t in tags])
    s2 = prob.solve()
    assert s2["setup_kind"] == lm.SETUP_LOAD            # reported truthfully: no append under the switch
    fresh, cam_f, caps_f, tags_f = build(None)
    cam_f[:] = start[0]
    for c, c0 in zip(caps_f, start[1]):
        c[:] = c0
    for t, t0 in zip(tags_f, start[2]):
        t[:] = t0
    for c in added:
        for b in np.nonzero(g.obs_cap == c)[0]:
            fresh.add_residual_block(g.corners[b], cam_f, caps_f[g.obs_cap[b]], tags_f[g.obs_tag[b]])
    s3 = fresh.solve()
    assert [i["step_is_successful"] for i in s2["iterations"]] == [i["step_is_successful"] for i in s3["iterations"]]
    for a, b in zip(s2["iterations"], s3["iterations"]):
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"]
    assert np.abs(camera[1:] - cam_f[1:]).max() <= L_TOL and abs(camera[0] - cam_f[0]) <= 1e-8 * cam_f[0]


# ---- 4. the scene of the README ----

def test_scene_from_a_zero_lens(lm, oracle):
    g = ref.scene()
    A = arrays(g)
    want = tref.solve(fref.FreeRadialOracle(oracle), fref.zero_lens(A))
    rp = lm.ResidentProblem(*fref.zero_lens(A), camera_model=lm.CAMERA_RADIAL, estimate_distortion=True)
    s = rp.solve()
    _assert_same((rp.camera, rp.cap, rp.tag, s), want)
    pin = lm.ResidentProblem(*A).solve()
    known = lm.ResidentProblem(*A, camera_model=lm.CAMERA_RADIAL)
    sk = known.solve()
    rms_f, rms_p, rms_k = (synth.rms_px(x["final_cost"], g.n_obs) for x in (s, pin, sk))
    rms_ref = synth.rms_px(want[3]["final_cost"], g.n_obs)
    print(f"scene l = {ref.SCENE} on the device, estimated from l = (0, 0): {len(s['iterations'])} iterations, "
          f"RMS {rms_f:.4f} px, f = {rp.camera[0]:.2f}, l1 = {rp.camera[1]:.4f}, l2 = {rp.camera[2]:.4f}; "
          f"with the known lens RMS {rms_k:.4f} px, f = {known.camera[0]:.2f}; as a pinhole RMS {rms_p:.4f} px")
    assert s["termination"] == "CONVERGENCE"
    assert rms_f <= 0.75 * rms_p
    assert abs(rp.camera[1] + 0.14) <= 0.02
    assert abs(rms_f - rms_ref) <= 1e-8 * rms_ref


# ---- 5. off is off ----

@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
def test_radial_without_the_switch_is_bit_for_bit_the_held_model(lm, with_loss):
    g = ref.trace_graphs(ref.MILD)["g20"][0]
    A, losses = arrays(g), _losses(g, with_loss)
    never = lm.ResidentProblem(*A, obs_loss=losses, camera_model=lm.CAMERA_RADIAL)
    s0 = never.solve()
    # set and cleared before the load
    cleared = lm.Problem()
    cleared.set_estimate_distortion(True)
    cleared.set_estimate_distortion(False)
    cleared.close()
    off = lm.ResidentProblem(*A, obs_loss=losses, camera_model=lm.CAMERA_RADIAL, estimate_distortion=False)
    on = lm.ResidentProblem(*A, obs_loss=losses, camera_model=lm.CAMERA_RADIAL, estimate_distortion=True)
    s_on = on.solve()
    on.set_estimate_distortion(False)                       # drops the loaded problem
    with pytest.raises(lm.LMError) as e:
        on.solve()
    assert e.value.code == -7
    s1 = off.solve()
    assert _trace(s1) == _trace(s0) and s1["final_cost"] == s0["final_cost"]
    assert np.array_equal(off.camera, never.camera) and np.array_equal(off.cap, never.cap) and np.array_equal(off.tag, never.tag)
    assert np.array_equal(off.camera[1:], ref.MILD)         # held, and handed back
    assert _trace(s_on) != _trace(s0)                       # (the switch does something)
    # a handle that had it on, cleared, then loads: the held model's bits again
    h = lm.Problem()
    h.set_camera_model(lm.CAMERA_RADIAL)
    h.set_estimate_distortion(True)
    h.set_estimate_distortion(False)
    k = lm.Problem()
    k.set_camera_model(lm.CAMERA_RADIAL)
    out = []
    for prob in (h, k):
        camera, caps, tags = A[0].copy(), [c.copy() for c in g.cap], [t.copy() for t in g.tag]
        for b in range(g.n_obs):
            prob.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]],
                                    loss=(CAUCHY, 3.0) if with_loss else None)
        out.append((_trace(prob.solve()), camera, np.array(caps), np.array(tags)))
    assert out[0][0] == out[1][0]
    assert all(np.array_equal(a, b) for a, b in zip(out[0][1:], out[1][1:]))


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
def test_pinhole_ignores_the_switch_bit_for_bit(lm, with_loss):
    g = ref.trace_graphs(ref.MILD)["g20"][0]
    A, losses = arrays(g), _losses(g, with_loss)
    a = lm.ResidentProblem(*A, obs_loss=losses)
    b = lm.ResidentProblem(*A, obs_loss=losses, estimate_distortion=True)
    sa, sb = a.solve(), b.solve()
    assert _trace(sb) == _trace(sa) and sb["final_cost"] == sa["final_cost"]
    assert np.array_equal(b.camera, a.camera) and np.array_equal(b.cap, a.cap) and np.array_equal(b.tag, a.tag)
    assert np.array_equal(b.camera[1:], ref.MILD)


# ---- 6. determinism ----

def test_two_solves_give_identical_bits(lm):
    g = ref.trace_graphs(ref.MILD)["gk11"][0]
    out = []
    for _ in range(2):
        rp = lm.ResidentProblem(*fref.zero_lens(arrays(g)), camera_model=lm.CAMERA_RADIAL, estimate_distortion=True)
        out.append((_trace(rp.solve()), rp.camera.copy(), rp.cap.copy(), rp.tag.copy(), rp.debug_camera_rows(1e4)[0]))
    assert out[0][0] == out[1][0]
    assert all(np.array_equal(a, b) for a, b in zip(out[0][1:], out[1][1:]))


# ---- 7. what the switch does not cover is refused ----

def test_several_ranks_are_refused(lm):
    g = ref.trace_graphs(ref.MILD)["g6"][0]
    rp = lm.ResidentProblem(*fref.zero_lens(arrays(g)), camera_model=lm.CAMERA_RADIAL, estimate_distortion=True)
    s0 = rp.solve()
    for call in (lambda: rp.debug_force_multirank(True), lambda: rp.set_comm(0, 2, lambda a, op: None)):
        with pytest.raises(lm.LMError) as e:
            call()
        assert e.value.code == UNSUPPORTED
        assert _trace(rp.solve()) == _trace(s0)             # the handle as it was: the loaded problem still solves
    multi = lm.Problem()
    multi.debug_force_multirank(True)
    multi.set_estimate_distortion(True)                     # (ignored under PINHOLE)
    with pytest.raises(lm.LMError) as e:
        multi.set_camera_model(lm.CAMERA_RADIAL)
    assert e.value.code == UNSUPPORTED and multi.camera_model() == lm.CAMERA_PINHOLE
    multi.set_estimate_distortion(False)
    multi.set_camera_model(lm.CAMERA_RADIAL)
    with pytest.raises(lm.LMError) as e:
        multi.set_estimate_distortion(True)
    assert e.value.code == UNSUPPORTED and multi.estimate_distortion() is False


def test_mixed_set_of_both_sides_is_refused(lm):
    g = tref.trace_graphs()["small"][0]                     # Ceres' set: 32 captures + 7 tags
    A = fref.zero_lens(arrays(g))
    info = lm.ResidentProblem(*A, elimination=lm.ELIM_MIXED).solve()
    assert info["ceres_e_captures"] > 0 and info["ceres_e_tags"] > 0
    camera, caps, tags = A[0].copy(), [c.copy() for c in g.cap], [t.copy() for t in g.tag]
    prob = lm.Problem(elimination=lm.ELIM_MIXED)
    prob.set_camera_model(lm.CAMERA_RADIAL)
    prob.set_estimate_distortion(True)
    for b in range(g.n_obs):
        prob.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]])
    with pytest.raises(lm.LMError) as e:
        prob.solve()
    assert e.value.code == UNSUPPORTED and "MIXED" in str(e.value)
    assert np.array_equal(camera, A[0])
    prob.set_options(elimination=lm.ELIM_AUTO)              # a supported solve on the same handle
    s = prob.solve()
    assert s["termination"] == "CONVERGENCE" and s["final_cost"] < s["initial_cost"]
    # a MIXED set that is one whole side is solved
    g6 = ref.trace_graphs(ref.MILD)["g6"][0]
    rp = lm.ResidentProblem(*fref.zero_lens(arrays(g6)), camera_model=lm.CAMERA_RADIAL, estimate_distortion=True,
                            elimination=lm.ELIM_MIXED)
    s6 = rp.solve()
    assert s6["elimination_used"] in (lm.ELIM_CAPTURES, lm.ELIM_TAGS) and abs(rp.camera[1]) > 1e-3


def test_covariances_are_refused(lm):
    g = ref.trace_graphs(ref.MILD)["g6"][0]
    rp = lm.ResidentProblem(*fref.zero_lens(arrays(g)), camera_model=lm.CAMERA_RADIAL, estimate_distortion=True)
    s0 = rp.solve()
    for call in (rp.covariance, lambda: rp.covariance_pairs([((lm.BLOCK_TAG, 0), (lm.BLOCK_TAG, 1))])):
        with pytest.raises(lm.LMError) as e:
            call()
        assert e.value.code == UNSUPPORTED
    assert _trace(rp.solve()) == _trace(s0)
