"""GPU tests: the stages of one LM step between the rows and the factorization, one at a time
(arslam_lm_debug_step_stages) against tests/step_ref.py's long-double reduction.

The whole-solve checks (traces to 1e-9, poses to 1e-6 m, goldens) cannot see one wrong
off-diagonal block of S, a dropped gather contribution, a wrong piece of a split destination or a
wrong W y_F term as long as the solve still converges: LM corrects a slightly wrong step.  Here
every output of k_lin_reduce / k_slot_norms / k_scale / k_lm_diag, k_schur<false> and <true>,
k_schur_gather / k_schur_combine (prep mode), k_schur_cam, k_update_f, k_backsub and the fused
candidate cost is held to the project's tolerance rule (test_gpu_tile_llt.py, test_gpu_lm_cov.py):

    e_dev <= 16 max(e_ref64, 2.3e-16),

both errors against numpy.longdouble, e_ref64 the float64 restatement of the same operation
(step_ref: the same sums per e-block, the explicit inverse of U, contributions in block order),
16 the rule's room for summation order and MFMA against BLAS.  The measures (DESIGN "Stage checks
of one step"): S by max |D_ij| / sqrt(H_ii H_jj), rhs by max |D_i| / (sqrt(H_ii) |r|), H the
un-eliminated diagonal; g by |D_i| / (sqrt(colnorm_i) |r|); colnorm, scale, diag relative; a
block's step by |D| / |step of the block|; the model change and the step^2 sums relative.  The
restatement's own S error is capped (CAPS: conditions on the inputs, so that a broken restatement
cannot loosen the bound).

The candidate cost is compared with the oracle's cost at the device's own candidate.  Its bound
comes from the row test (test_gpu_parity.py: a device residual is within 1e-12 |r| + 1e-9 of the
oracle's): with rho' <= 1 for every loss, |D cost| <= sum |r_i| e_i + e_i^2 / 2
<= 1e-12 sum r_i^2 + 1e-9 sum |r_i| (+ 1e-18 per row), plus the summation's 8 nb 2^-53 cost.

Every case prints a line starting `step_stages:` (the MI355X record:
profiles/step_stages/device_errors.txt).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import step_ref as sr  # noqa: E402
import tag_size_ref as tref  # noqa: E402
from ar_slam_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

RULE = 16.0


# ---- inputs (step_ref's: the CPU test holds the restatement's floors on the same ones) ----

_spec = sr.spec
_LATE_SPECS = sr.LATE_SPECS
CAPS = sr.CAPS


def _arrays(s):
    return tref.arrays(s["g"])


@functools.lru_cache(maxsize=None)
def _rows(name, oracle):
    """The reference's problem and rows at the loaded point (shared by every case of a name)."""
    P = sr.spec_problem(oracle, name)
    R = sr.Rows(P)
    g, cn, rr = sr.sums(R)
    g64, cn64, _ = sr.sums(R, np.float64)
    return P, R, (g, cn, rr), (g64, cn64, *sr.sum_floors(R, g, cn, rr))


@functools.lru_cache(maxsize=None)
def _reference(name, oracle, elim_bytes, radius):
    """The long-double reduced system, the float64 restatement and the restatement's errors."""
    P, R, (g, cn, rr), (g64, cn64, _, _) = _rows(name, oracle)
    elim = np.frombuffer(elim_bytes, bool)
    s, d = sr.scale_diag(P, cn)
    s64, d64 = sr.scale_diag(P, cn64, dtype=np.float64)
    ref = sr.reduce(R, elim, s, d, radius, True)
    r64 = sr.reduce(R, elim, s64, d64, radius, False)
    return dict(s=s, d=d, s64=s64, d64=d64, ref=ref, e64=sr.errors(r64.S, r64.rhs, ref))


@functools.lru_cache(maxsize=4)
def _reduce_at(name, oracle, elim_bytes, scale_bytes, diag_bytes, radius):
    """The reduction from a device's own scale and diagonal, long double and float64 (two outputs
    with the same bits of both -- a sharded step's two exchange modes -- share it)."""
    R = _rows(name, oracle)[1]
    elim, scale, diag = np.frombuffer(elim_bytes, bool), np.frombuffer(scale_bytes), np.frombuffer(diag_bytes)
    return sr.reduce(R, elim, scale, diag, radius, True), sr.reduce(R, elim, scale, diag, radius, False)


def _load(lm, name, **opts):
    s = _spec(name)
    kw = {}
    if s["loss"]:
        kw["loss"] = s["loss"]
    if s["sizes"] is not None:
        kw["tag_size"] = s["sizes"]
    if s["model"] != "pinhole":
        kw["camera_model"] = lm.CAMERA_RADIAL
    if s["model"] == "radial_est":
        kw["estimate_distortion"] = True
    return lm.ResidentProblem(*_arrays(s), s["camera_const"], s["cap_const"], s["tag_const"], **kw, **opts)


# ---- the measures ----

def _rel(a, ref, mask=None):
    """max |a - ref| / |ref| over the entries (of mask) where ref != 0; where it is 0 so is a."""
    a, ref = np.asarray(a, sr.LD), np.asarray(ref, sr.LD)
    mask = np.ones(ref.shape, bool) if mask is None else mask
    m, z = mask & (ref != 0), mask & (ref == 0)
    assert np.all(a[z] == 0)
    return float(np.max(np.abs(a[m] - ref[m]) / np.abs(ref[m]))) if m.any() else 0.0


def _bound(e64):
    return RULE * max(float(e64), sr.FLOOR)


def _block_err(delta, ref_delta, P, slack=None):
    """max over the pose blocks and the camera of (|D| - slack) / |the block's reference step|
    (slack [n]: an absolute allowance per slot, taken off in norm)."""
    worst = 0.0
    blocks = [np.arange(3)] + [sr.block_slots(P, b) for b in range(P.nc + P.nt)]
    for sl in blocks:
        nrm = float(np.sqrt(np.sum(ref_delta[sl] ** 2)))
        if nrm > 0:
            err = float(np.sqrt(np.sum((np.asarray(delta[sl], sr.LD) - ref_delta[sl]) ** 2)))
            if slack is not None:
                err = max(0.0, err - float(np.sqrt(np.sum(slack[sl] ** 2))))
            worst = max(worst, err / nrm)
    return worst


def _plain_cost_terms(P, x):
    """(sum r^2, sum |r|, rows) of the uncorrected residuals at x: the candidate cost's bound."""
    cam, cap, tag = P.unpack(x)
    s2 = s1 = 0.0
    for o in range(P.nb):
        r = tref.residual(P.oracle, cam, cap[P.obs_cap[o]], tag[P.obs_tag[o]], P.corners[o], P.size[o])
        s2 += float(r @ r)
        s1 += float(np.sum(np.abs(r)))
    return s2, s1, 8 * P.nb


def _block_rows(out, P):
    """The first reduced row of each of the caller's blocks (captures, then tags), -1 for none."""
    rows = np.full(P.nc + P.nt, -1)
    for r, sl in enumerate(out["row_slot"]):
        if sl >= 3 and (sl - 3) % 6 == 0:
            rows[(sl - 3) // 6] = r
    return rows


def check_case(lm, oracle, name, radius, label, expect=None, handle=None, **opts):
    """One loaded problem, one radius: every stage output against the reference.  Returns the
    device's outputs and the figures (also printed).  handle: a problem already loaded (else
    the named one is loaded with opts)."""
    rp = handle if handle is not None else _load(lm, name, **opts)
    out = rp.debug_step_stages(radius)
    P = _rows(name, oracle)[0]
    assert out["n"] == P.n
    if expect:
        expect(out)
    if hasattr(rp, "debug_reduced_rows"):   # arslam_lm_debug_reduced_rows says the same, a mixed set included
        cap_row, tag_row, cam_row = rp.debug_reduced_rows()
        assert np.array_equal(np.concatenate([cap_row, tag_row]), _block_rows(out, P)) and cam_row == out["cam_row"]
    fig = stage_figures(name, oracle, radius, out)
    report("step_stages", name, label, radius, out["n_reduced"], fig)
    return rp, out


def reference_of(name, oracle, radius, out):
    """The reference of the elimination the device's reduced rows (out["row_slot"]) say."""
    P = _rows(name, oracle)[0]
    rows = _block_rows(out, P)
    elim = sr.e_set(P, rows[:P.nc], rows[P.nc:])
    return elim, _reference(name, oracle, elim.tobytes(), float(radius))


def lin_figures(name, oracle, c, out, fr=None, sm=None):
    """The linearization's sums, the scale, the LM diagonal of one output, over the free slots fr
    (default: all of them; the scale over sm, default every slot).  Returns (figures, g's floor)."""
    P, R, (g, cn, rr), (g64, cn64, g_floor, cn_floor) = _rows(name, oracle)
    fig = {}
    rn = np.sqrt(rr)
    gden = np.where(cn > 0, np.sqrt(cn) * rn, 1)
    fr = P.free if fr is None else fr
    # (the restatement's floor takes in the rounding of the rows themselves, which the device
    # performs and the restatement, sharing the reference's rows, does not: step_ref.Rows.rerr
    # and wrel, by slot for g and colnorm; scale = 1 / (1 + sqrt(colnorm)) carries at most half
    # of colnorm's, diag = s^2 colnorm at most all of it; rhs twice g's; the model change its own)
    gf, cf = float(np.max(g_floor[fr])), float(np.max(cn_floor[fr]))
    fig["g"] = (float(np.max((np.abs(out["g"] - g) / gden)[fr])), float(np.max((np.abs(g64 - g) / gden)[fr])) + gf)
    fig["colnorm"] = (_rel(out["colnorm"], cn, fr), _rel(cn64, cn, fr) + cf)
    fig["scale"] = (_rel(out["scale"], c["s"], sm), _rel(c["s64"], c["s"], sm) + 0.5 * cf)
    fig["diag"] = (_rel(out["diag"], c["d"], fr), _rel(c["d64"], c["d"], fr) + cf)
    return fig, gf


def stage_figures(name, oracle, radius, out, padded=True, system_floor=None):
    """{stage: (e_dev, e_ref64)} of one step's outputs `out` (debug_step_stages' keys) against the
    reference, with every exact property asserted on the way.  padded=False: out has no
    S_padded to look at (a system summed from the ranks' shares); system_floor = (e_S, e_rhs):
    the restatement's errors to hold S and rhs to instead of the one-level restatement's."""
    spec = _spec(name)
    P, R, (g, cn, rr), (g64, cn64, g_floor, cn_floor) = _rows(name, oracle)
    elim, c = reference_of(name, oracle, radius, out)
    ref = c["ref"]
    e64 = c["e64"] if system_floor is None else system_floor

    # -- the linearization's sums, the scale, the LM diagonal
    fig, gf = lin_figures(name, oracle, c, out)

    # -- the assembled system
    nR, N = out["n_reduced"], out["n_padded"]
    slot = out["row_slot"]
    if spec["camera_const"]:
        assert out["cam_row"] == -1 and not np.any((slot >= 0) & (slot < 3))
    if len(ref.slots):
        real = np.nonzero(slot >= 0)[0]
        assert sorted(slot[real].tolist()) == ref.slots.tolist(), "the reduced rows are the free f-side slots"
        row_of = np.full(P.n, -1)
        row_of[slot[real]] = real
        ix = row_of[ref.slots]
        S_dev, rhs_dev = out["S"][np.ix_(ix, ix)], out["rhs"][ix]
        assert np.array_equal(out["S"], out["S"].T)
        fig["S"] = (sr.errors(S_dev, rhs_dev, ref)[0], e64[0])
        fig["rhs"] = (sr.errors(S_dev, rhs_dev, ref)[1], e64[1] + 2 * gf)
        assert fig["S"][1] <= CAPS[float(radius)], f"the restatement's own S error {fig['S'][1]:.2e}: replace the input"
        # exactly zero wherever no e-block couples the two blocks, fill tiles included
        assert np.all(S_dev[~ref.struct] == 0.0)
        if padded:
            # the padding rows are identity rows, the right-hand side's row has its pivot and nothing after it
            Sp = out["S_padded"]
            pad = np.concatenate([np.nonzero(slot < 0)[0], np.arange(nR + 1, N)])
            eye = np.eye(N)
            assert np.array_equal(Sp[pad], eye[pad]) and np.array_equal(Sp[:, pad], eye[:, pad])
            assert Sp[nR, nR] == 1e300
        # the diagonal carries D^2: where nothing else lands it is D^2 alone, bit for bit
        d2 = np.sqrt(out["diag"] / radius) ** 2
        lone = np.nonzero(np.asarray(ref.H - ref.D2[ref.slots] == 0))[0]
        assert np.array_equal(np.diag(S_dev)[lone], d2[ref.slots[lone]])
    else:
        assert nR == 0 and N == 0

    # -- the step.  A failed pivot is LM's invalid step (the radius shrinks): nothing after the
    # factorization means anything then.  It is accepted only at radius 1e16, where D^2 ~ 1e-22
    # leaves the gauge freedom of the problem in S, and only if the reference's S says so too.
    if out["indefinite"]:
        assert radius == 1e16
        w = np.linalg.eigvalsh(np.asarray(ref.S, np.float64))
        assert w[0] <= len(w) * sr.U64 * w[-1], "the device calls a well-conditioned system indefinite"
    else:
        assert not out["e_step_bad"] and not out["f_step_bad"] and not out["candidate_bad"]
        if len(ref.slots):
            # y by the normwise backward error on the device's own S, beside LAPACK's on the same S
            def eta(y):
                res = np.asarray(S_dev, sr.LD) @ np.asarray(y, sr.LD) - np.asarray(rhs_dev, sr.LD)
                return float(np.max(np.abs(res)) / (np.max(np.sum(np.abs(S_dev), axis=1)) * np.max(np.abs(y)) +
                                                   np.max(np.abs(rhs_dev))))
            Lc = np.linalg.cholesky(S_dev)
            fig["y"] = (eta(out["y"][ix]), eta(np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs_dev))))
        # -- the candidate, from the device's own y and scale
        red_ld, red_64 = _reduce_at(name, oracle, elim.tobytes(), out["scale"].tobytes(), out["diag"].tobytes(),
                                    float(radius))
        y_dev = out["y"][ix] if len(ref.slots) else np.zeros(0)
        st = sr.back_substitute(R, red_ld, y_dev, out["scale"], True)
        st64 = sr.back_substitute(R, red_64, y_dev, out["scale"], False)
        x0 = P.x0
        assert np.array_equal(out["xc"][~P.free], x0[~P.free]), "constant and unused slots keep their bits"
        # The entry returns x + d, not d: the stored sum is off by at most half an ulp of itself per
        # slot.  That rounding is taken off the measured error by its bound (it is the number
        # format's, not the stage's): per block in norm, and for a sum of squares
        # |sum (d + e)^2 - sum d^2| <= 2 |d| |e| + |e|^2.
        d_dev = out["xc"] - x0
        slack = sr.U64 * np.abs(out["xc"])
        fig["step"] = (_block_err(d_dev, st.delta, P, slack), _block_err(st64.delta, st.delta, P))
        fig["model"] = (abs(out["model_cost_change"] - float(st.model)) / abs(float(st.model)),
                        (abs(float(st64.model - st.model)) + st.model_floor) / abs(float(st.model)))
        f_slots = np.zeros(P.n, bool)
        f_slots[ref.slots] = True
        for k, part in (("e_step2", P.free & ~f_slots), ("f_step2", f_slots)):
            want = float(getattr(st, k))
            if want > 0:
                e = float(np.sqrt(np.sum(slack[part] ** 2)))
                off = (2 * np.sqrt(want) * e + e * e) / want
                fig[k] = (max(0.0, abs(out[k] - want) / want - off), abs(float(getattr(st64, k)) - want) / want)
            else:
                assert out[k] == 0.0

        # -- the candidate's cost, at the device's own candidate
        act, fix, ok = P.cost(out["xc"])
        s2, s1, rows = _plain_cost_terms(P, out["xc"])
        cost_bound = 1e-12 * s2 + 1e-9 * s1 + 1e-18 * rows + rows * sr.U64 * (act + fix)
        fig["cost"] = (abs(out["candidate_cost"] - act) + abs(out["candidate_fixed_cost"] - fix), cost_bound)
    return fig


def report(prefix, name, label, radius, nR, fig):
    """Print the case's line (e_dev / e_ref64 per stage, the worst e_dev / bound) and hold every
    stage to the rule; the candidate cost to its own bound."""
    worst = {}
    for k, (e_dev, e_ref) in fig.items():
        b = e_ref if k == "cost" else _bound(e_ref)
        worst[k] = e_dev / b
    print("%s: %-16s %-10s r=%-6g nR=%-4d " % (prefix, name, label, radius, nR) +
          " ".join("%s %.1e/%.1e" % (k, v[0], v[1]) for k, v in fig.items()) +
          "  worst %s %.2f" % max(((k, v) for k, v in worst.items()), key=lambda kv: kv[1]))
    for k, v in worst.items():
        assert v <= 1.0, f"{name} {label} radius {radius}: {k} e_dev {fig[k][0]:.3e} over its bound ({v:.2f} x)"


def _same_bits(a, b):
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, b[k]), k
        else:
            assert v == b[k], k


# ---- the cases ----

@pytest.mark.parametrize("radius", [1e-2, 1e4, 1e16])
@pytest.mark.parametrize("name", ["k1to11", "small"])
def test_every_output_shape_of_the_schur_kernel(lm, oracle, name, radius):
    """The k1to11 graph (44 captures of 1..11 tags): every shape of the 13-tile MFMA output, one
    capture on k_schur<true>, two observation chunks; and `small`.  All three radius classes."""
    def expect(o):
        if name == "k1to11":
            assert o["n_big_groups"] >= 1 and o["n_chunk_groups"] >= 1
    check_case(lm, oracle, name, radius, "captures", expect, elimination=lm.ELIM_CAPTURES)


@pytest.mark.parametrize("radius", [1e-2, 1e4])
def test_constant_tag_and_camera_on_the_k1to11_graph(lm, oracle, radius):
    check_case(lm, oracle, "k1to11_const", radius, "captures", elimination=lm.ELIM_CAPTURES)


@pytest.mark.parametrize("radius", [1e-2, 1e4])
def test_a_capture_of_thirty_tags(lm, oracle, radius):
    def expect(o):
        assert o["n_big_groups"] == 1
    check_case(lm, oracle, "k30", radius, "captures", expect, elimination=lm.ELIM_CAPTURES)


@pytest.mark.parametrize("radius", [1e-2, 1e4])
@pytest.mark.parametrize("name,most", [("pair70", 70), ("pair170", 170), ("single1030", 1030)])
def test_split_gather_destinations(lm, oracle, name, most, radius):
    """Destinations summed in pieces (k_schur_gather's partial sums, k_schur_combine): 70 > 64
    contributions of a 36-element block, 170 > 160 of a 6-element one, 1030 > 1024 of a scalar."""
    def expect(o):
        assert o["max_contrib"] == most and o["n_split_dest"] >= 1 and np.count_nonzero(o["row_slot"] >= 0) == 15
    check_case(lm, oracle, name, radius, "captures", expect, elimination=lm.ELIM_CAPTURES)


@pytest.mark.parametrize("radius", [1e-2, 1e4, 1e16])
@pytest.mark.parametrize("side", ["tags", "mixed"])
def test_tag_and_mixed_elimination(lm, oracle, side, radius):
    """`small` with the tags eliminated (a plan with alignment padding rows) and with Ceres' mixed
    set (direct groups: residuals with both poses on the reduced side)."""
    def expect(o):
        if side == "tags":
            assert o["elimination_used"] == lm.ELIM_TAGS
            assert np.count_nonzero(o["row_slot"] < 0) > 0, "no alignment padding rows"
        else:
            assert o["elimination_used"] == lm.ELIM_MIXED and o["n_direct"] >= 1
    check_case(lm, oracle, "small", radius, side, expect,
               elimination=lm.ELIM_TAGS if side == "tags" else lm.ELIM_MIXED)


@pytest.mark.parametrize("radius", [1e-2, 1e4])
@pytest.mark.parametrize("name", ["small_cauchy", "small_sized", "g20_radial", "g20_radial_est", "g20_cap_const",
                                  "g20_tag_const", "g20_camera_const", "g20_f_const"])
def test_losses_sides_models_and_constant_blocks(lm, oracle, name, radius):
    """Cauchy loss on outliers; mixed tag sides; the radial model held and with l1, l2 estimated
    (the whole system, not only the camera's three rows); a constant capture, tag, camera; and
    the camera with every tag constant (no reduced system: k_backsub's own inv6 path)."""
    def expect(o):
        if name == "g20_f_const":
            assert o["n_reduced"] == 0
        if name == "g20_radial_est":
            assert np.all(o["colnorm"][1:3] > 0)
    check_case(lm, oracle, name, radius, "auto", expect)


@pytest.mark.parametrize("name", ["k1to11", "small"])
def test_both_factor_executors(lm, oracle, name):
    """y, the candidate and the scalars from the level launches as from the persistent executor."""
    for ex in (0, 1):
        check_case(lm, oracle, name, 1e4, f"executor{ex}", elimination=lm.ELIM_CAPTURES, factor_executor=ex)


@pytest.mark.parametrize("name,elimination", [("k1to11", 1), ("small", 3), ("g20_radial_est", 0)])
def test_repeatable_and_invisible_to_the_next_solve(lm, oracle, name, elimination):
    """Two calls return the same bits, and the solve after them the bits of a fresh handle's."""
    rp = _load(lm, name, elimination=elimination)
    a = rp.debug_step_stages(1e4)
    b = rp.debug_step_stages(1e4)
    _same_bits(a, b)
    rp.debug_step_stages(1e-2)
    s1 = rp.solve()
    fresh = _load(lm, name, elimination=elimination)
    s2 = fresh.solve()
    assert [i["cost"] for i in s1["iterations"]] == [i["cost"] for i in s2["iterations"]]
    assert s1["final_cost"] == s2["final_cost"]
    assert np.array_equal(rp.camera, fresh.camera) and np.array_equal(rp.cap, fresh.cap)
    assert np.array_equal(rp.tag, fresh.tag)


def test_appended_coupling_in_a_fill_tile(lm, oracle):
    """A pointer-keyed problem after an append whose coupling lands in a fill tile of the loaded
    factor (the setup of test_gpu_parity's test of that name, on `wide`): the extended gather
    writes a tile no capture of the load touched, and every stage is still the grown problem's."""
    g = synth.config_graph("wide")
    first = 250
    camera = g.camera.copy()
    caps = [g.cap[c].copy() for c in range(first)]
    tags = [g.tag[t].copy() for t in range(g.n_tag)]
    prob = lm.Problem(elimination=lm.ELIM_CAPTURES, max_num_iterations=2)
    seen, pairs = set(), set()
    for c in range(first):
        ts = sorted(set(g.obs_tag[g.obs_cap == c].tolist()))
        seen.update(ts)
        pairs.update((a, b) for a in ts for b in ts if a < b)
    obs = [(g.corners[b], int(g.obs_cap[b]), int(g.obs_tag[b])) for b in range(g.n_obs) if g.obs_cap[b] < first]
    for corners, c, t in obs:
        prob.add_residual_block(corners, camera, caps[c], tags[t])
    assert prob.solve()["setup_kind"] == lm.SETUP_LOAD
    xy = g.tag_true[:, :2]
    hist, fill = {}, []
    for a in sorted(seen):
        for b in sorted(seen):
            d = np.linalg.norm(xy[a] - xy[b])
            if a >= b or (a, b) in pairs or d > 3.0:
                continue
            st = prob.debug_tag_pair_tile(tags[a], tags[b])
            hist[st] = hist.get(st, 0) + 1
            if st == 1:
                fill.append((d, a, b))
    assert fill, f"no unseen tag pair in a fill tile (pair statuses {hist})"
    _, a, b = sorted(fill)[0]
    rng = np.random.default_rng(5)
    mid = 0.5 * (g.tag_true[a, :3] + g.tag_true[b, :3])
    h = max(2.0, 1.1 * np.linalg.norm(xy[a] - xy[b]))
    pose = np.array([-mid[0], -mid[1], h, 0.0, 0.0, 0.0])
    cor = synth.project_corners(g.camera_true, np.tile(pose, (2, 1)), g.tag_true[[a, b]])
    cor = cor + rng.normal(0.0, 0.5, cor.shape)
    caps.append(pose + rng.normal(0, 0.02, 6))
    for row, t in zip(cor, (a, b)):
        obs.append((np.ascontiguousarray(row), len(caps) - 1, t))
        prob.add_residual_block(obs[-1][0], camera, caps[-1], tags[t])
    # the loaded point of the second solve; blocks in the order they were first added
    tag_order = list(dict.fromkeys(t for _, _, t in obs))
    tpos = {t: i for i, t in enumerate(tag_order)}
    arrays = (camera.copy(), np.array(caps), np.array([tags[t] for t in tag_order]),
              np.array([c for _, c, _ in obs], np.int32), np.array([tpos[t] for _, _, t in obs], np.int32),
              np.array([c for c, _, _ in obs]))
    assert prob.solve()["setup_kind"] == lm.SETUP_APPEND
    s = dict(camera_const=False, cap_const=None, tag_const=None, sizes=None, loss=None, model="pinhole")
    s["g"] = synth.Graph(*arrays, None, None, None, "wide_appended")
    _LATE_SPECS["wide_appended"] = s

    def expect(o):
        assert o["n_tiles"] > o["n_assembled_tiles"]
    for radius in (1e-2, 1e4):
        _, out = check_case(lm, oracle, "wide_appended", radius, "appended", expect, handle=prob)
    # the pair's block is there: the reference's, non-zero, in a tile the load did not assemble
    ra, rb = (int(np.nonzero(out["row_slot"] == 3 + 6 * (first + 1) + 6 * tpos[t])[0][0]) for t in (a, b))
    assert prob.debug_tag_pair_tile(tags[a], tags[b]) == 1 and np.all(out["S"][ra:ra + 6, rb:rb + 6] != 0)
