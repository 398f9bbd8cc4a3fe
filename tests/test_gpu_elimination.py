"""GPU parity of the elimination sides and of Ceres' exact mixed set
(arslam_lm_options.elimination).

DENSE_SCHUR eliminates Ceres' own e-block set (ar_slam_util.cpp:1011; Ceres
2.0 ComputeStableSchurOrdering): mostly tags on the demo-sized cfg1 graph and
early incremental graphs, mostly captures on the benchmark graphs.  The
device eliminates one whole side -- the majority side of that set under
ARSLAM_ELIM_AUTO -- by running its per-e-block kernels on the role-swapped
problem (captures become the reduced system).  Either side is the same exact
solve of the same LM system, so both must reproduce the oracle's trace
(capture elimination) to rounding: per-iteration cost 1e-9, final cost and
focal 1e-8, same termination, every gauge-aligned capture and tag pose
1e-6 m / 1e-7 rad (tests/gauge.py).  ELIM_MIXED eliminates exactly
Ceres' set, captures and tags together, and is checked against the
oracle eliminating the same set (OR_ELIM_MIXED) at the same tolerances.
"""
import json
import os

import numpy as np
import pytest

from ar_slam_amd import synth
from gauge import assert_poses_match
from oracle.schur_ordering import ceres_e_blocks
from test_gpu_parity import assert_matches_fresh_load

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _compare(g, ours, ref):
    cam_o, cap_o, tag_o, s_o = ours
    cam_r, cap_r, tag_r, s_r = ref
    assert (s_o["termination"], s_o["rule"]) == (s_r["termination"], s_r["rule"])
    assert abs(len(s_o["iterations"]) - len(s_r["iterations"])) <= 1
    for a, b in list(zip([i["cost"] for i in s_o["iterations"]], [i["cost"] for i in s_r["iterations"]]))[:5]:
        assert abs(a - b) <= 1e-9 * abs(b)
    assert abs(s_o["final_cost"] - s_r["final_cost"]) <= 1e-8 * s_r["final_cost"]
    assert abs(cam_o[0] - cam_r[0]) <= 1e-8 * cam_r[0]
    assert_poses_match(cap_o, tag_o, cap_r, tag_r, tags=np.unique(g.obs_tag), caps=np.unique(g.obs_cap))


@pytest.mark.parametrize("side", ["captures", "tags", "auto"])
@pytest.mark.parametrize("name", ["cfg1", "tiny", "small", "medium", "wide"])
def test_both_sides_match_oracle(lm, oracle, name, side):
    g = synth.config_graph(name)
    elim = {"auto": lm.ELIM_AUTO, "captures": lm.ELIM_CAPTURES, "tags": lm.ELIM_TAGS}[side]
    ours = lm.solve_graph(g, elimination=elim)
    ref = oracle.solve_graph(g)
    _compare(g, ours, ref)
    s = ours[3]
    rule = ceres_e_blocks(g.obs_cap, g.obs_tag, g.n_cap, g.n_tag)
    assert (s["ceres_e_captures"], s["ceres_e_tags"]) == (rule["captures"], rule["tags"])
    if side == "auto":
        side = "tags" if rule["tags"] > rule["captures"] else "captures"
    assert s["elimination_used"] == {"captures": lm.ELIM_CAPTURES, "tags": lm.ELIM_TAGS}[side]
    # the reduced system is the other side plus the camera
    n_f = g.n_cap if side == "tags" else len(np.unique(g.obs_tag))
    assert s["n_reduced"] >= 6 * n_f + 1


@pytest.mark.parametrize("side", ["tags", "mixed"])
@pytest.mark.parametrize("name", ["tiny_reject", "small_reject", "tiny_failure", "small_parameter"])
def test_control_traces_under_tag_elimination(lm, name, side):
    """Rejected steps, invalid steps -> FAILURE and the parameter rule, with tags eliminated, and
    with Ceres' exact set (all tags on tiny, captures and tags together on small)."""
    with open(os.path.join(GOLDEN, f"lm_ctl_{name}.json")) as f:
        gold = json.load(f)
    g = synth.config_graph(gold["config"], **gold["graph"])
    opts = dict(gold["options"])
    mask = opts.pop("debug_indefinite_mask", 0)
    elim = lm.ELIM_TAGS if side == "tags" else lm.ELIM_MIXED
    rp = lm.ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, elimination=elim, **opts)
    rp.debug_force_indefinite(mask)
    s = rp.solve()
    its = s["iterations"]
    ec, et = _ceres_set(g)
    assert s["elimination_used"] == (lm.ELIM_TAGS if side == "tags" or not ec.sum() else lm.ELIM_MIXED)
    assert (s["termination"], s["rule"]) == (gold["termination"], gold["rule"])
    assert [it["step_is_valid"] for it in its] == gold["step_is_valid"]
    assert [it["step_is_successful"] for it in its] == gold["step_is_successful"]
    ours = np.array([it["cost"] for it in its])
    ref = np.array(gold["cost"])
    alt = np.array(gold["alt_cost"])
    tol = np.maximum(1e-9, 20.0 * np.abs(alt - ref) / np.abs(ref))
    assert np.all(np.abs(ours - ref) / np.abs(ref) <= tol)


def test_pointer_api_under_tag_elimination(lm):
    """Caller-owned blocks are written back to the right places when the device problem is
    role-swapped; re-solving reloads values only."""
    g = synth.config_graph("tiny")
    outs = []
    for elim in (lm.ELIM_CAPTURES, lm.ELIM_TAGS):
        camera = g.camera.copy()
        caps = [g.cap[c].copy() for c in range(g.n_cap)]
        tags = [g.tag[t].copy() for t in range(g.n_tag)]
        prob = lm.Problem(elimination=elim)
        for b in range(g.n_obs):
            prob.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]])
        s = prob.solve()
        assert s["elimination_used"] == elim
        s2 = prob.solve()   # from the solved state: values-only reload
        assert s2["setup_kind"] == lm.SETUP_VALUES
        outs.append((camera, np.stack(caps), np.stack(tags), s))
    (c1, k1, t1, s1), (c2, k2, t2, s2) = outs
    assert abs(s1["final_cost"] - s2["final_cost"]) <= 1e-9 * s1["final_cost"]
    np.testing.assert_allclose(c1, c2, rtol=1e-8)
    np.testing.assert_allclose(k1[:, :3] - k1[:, :3].mean(0), k2[:, :3] - k2[:, :3].mean(0), atol=1e-6)


def _graph(name):
    g = synth.config_graph(name.split("[")[0])
    return synth.prefix_graph(g, int(name.split("[:")[1][:-1])) if "[:" in name else g


def _ceres_set(g, **kw):
    m = ceres_e_blocks(g.obs_cap, g.obs_tag, g.n_cap, g.n_tag, members=True, **kw)
    return np.array(m["e_cap"], np.uint8), np.array(m["e_tag"], np.uint8)


@pytest.mark.parametrize("name", ["cfg1", "small", "medium", "wide", "cfg2[:300]"])
def test_mixed_set_matches_oracle(lm, oracle, name):
    """ELIM_MIXED eliminates exactly Ceres' set (captures and tags together; cfg1's is all
    tags, the others mix), against the oracle eliminating the same set: the same trace at
    the tolerances above, every gauge-aligned pose."""
    g = _graph(name)
    ec, et = _ceres_set(g)
    ours = lm.solve_graph(g, elimination=lm.ELIM_MIXED)
    if ec.sum() and et.sum():
        ref = oracle.solve_graph(g, elimination=oracle.ELIM_MIXED, e_cap=ec, e_tag=et)
        used = lm.ELIM_MIXED
    else:
        ref = oracle.solve_graph(g)
        used = lm.ELIM_TAGS if et.sum() else lm.ELIM_CAPTURES
    _compare(g, ours, ref)
    s = ours[3]
    assert s["elimination_used"] == used
    assert s["n_owned_captures"] == g.n_cap   # (one rank: every capture, whatever the device groups)
    assert (s["ceres_e_captures"], s["ceres_e_tags"]) == (int(ec.sum()), int(et.sum()))
    # the reduced system: every capture and tag outside the set, and the camera
    n_f = g.n_cap + len(np.unique(g.obs_tag)) - int(ec.sum()) - int(et.sum())
    assert s["n_reduced"] >= 6 * n_f + 3


def test_mixed_set_with_constant_blocks(lm, oracle):
    """Constant captures and tags are not in Ceres' graph: the mixed set of what is left,
    constant blocks on the reduced side (no rows), against the oracle."""
    g = synth.config_graph("medium")
    rng = np.random.default_rng(11)
    cap_const = (rng.random(g.n_cap) < 0.1).astype(np.uint8)
    tag_const = (rng.random(g.n_tag) < 0.1).astype(np.uint8)
    kw = dict(cap_const=cap_const, tag_const=tag_const)
    ec, et = _ceres_set(g, **kw)
    assert ec.sum() and et.sum()
    ours = lm.solve_graph(g, elimination=lm.ELIM_MIXED, **kw)
    ref = oracle.solve_graph(g, elimination=oracle.ELIM_MIXED, e_cap=ec, e_tag=et, **kw)
    _compare(g, ours, ref)
    assert ours[3]["elimination_used"] == lm.ELIM_MIXED
    np.testing.assert_array_equal(ours[1][cap_const == 1], g.cap[cap_const == 1])
    np.testing.assert_array_equal(ours[2][tag_const == 1], g.tag[tag_const == 1])


def test_pointer_api_under_mixed_elimination(lm):
    """Caller-owned blocks are written back through the regrouping (eliminated captures and
    tags, the reduced side's captures and tags); a re-solve reloads values only and ends
    where a capture-eliminating solve ends."""
    g = synth.config_graph("small")
    outs = []
    for elim in (lm.ELIM_CAPTURES, lm.ELIM_MIXED):
        camera = g.camera.copy()
        caps = [g.cap[c].copy() for c in range(g.n_cap)]
        tags = [g.tag[t].copy() for t in range(g.n_tag)]
        prob = lm.Problem(elimination=elim)
        for b in range(g.n_obs):
            prob.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]])
        s = prob.solve()
        assert s["elimination_used"] == elim
        s2 = prob.solve()
        assert s2["setup_kind"] == lm.SETUP_VALUES
        outs.append((camera, np.stack(caps), np.stack(tags), s))
    (c1, k1, t1, s1), (c2, k2, t2, s2) = outs
    assert abs(s1["final_cost"] - s2["final_cost"]) <= 1e-9 * s1["final_cost"]
    np.testing.assert_allclose(c1, c2, rtol=1e-8)
    assert_poses_match(k2, t2, k1, t1, tags=np.arange(g.n_tag), caps=np.arange(g.n_cap))


def test_append_under_mixed_that_fell_back_to_captures(lm):
    """ELIM_MIXED on a graph whose Ceres set is every capture and no tag (six captures that each
    see the same four tags: a capture's degree is below a tag's, so the greedy independent set
    takes the captures) loads with the captures eliminated.  A seventh capture on those tags is
    then appended through the capture form of the append path (setup_kind APPEND) and the solve
    gives what a fresh handle's load of the grown problem gives."""
    g = synth.make_graph(7, 2, 2, seed=5, k=4)
    first = 6
    loaded = g.obs_cap < first
    rule = ceres_e_blocks(g.obs_cap[loaded], g.obs_tag[loaded], first, g.n_tag)
    assert (rule["captures"], rule["tags"]) == (first, 0)
    camera = g.camera.copy()
    caps = [g.cap[c].copy() for c in range(g.n_cap)]
    tags = [g.tag[t].copy() for t in range(g.n_tag)]
    prob = lm.Problem(elimination=lm.ELIM_MIXED)
    order = list(np.nonzero(loaded)[0]) + list(np.nonzero(~loaded)[0])
    for b in order[:int(loaded.sum())]:
        prob.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]])
    s1 = prob.solve()
    assert s1["ceres_e_tags"] == 0
    assert s1["elimination_used"] == lm.ELIM_CAPTURES
    assert s1["setup_kind"] == lm.SETUP_LOAD
    for b in order[int(loaded.sum()):]:
        prob.add_residual_block(g.corners[b], camera, caps[g.obs_cap[b]], tags[g.obs_tag[b]])
    start = (camera.copy(), [c.copy() for c in caps], [t.copy() for t in tags])
    s2 = prob.solve()
    assert s2["setup_kind"] == lm.SETUP_APPEND, s2["setup_kind"]
    fresh = lm.Problem(elimination=lm.ELIM_MIXED)
    cam_f, caps_f, tags_f = start[0].copy(), [c.copy() for c in start[1]], [t.copy() for t in start[2]]
    for b in order:
        fresh.add_residual_block(g.corners[b], cam_f, caps_f[g.obs_cap[b]], tags_f[g.obs_tag[b]])
    s3 = fresh.solve()
    assert s3["setup_kind"] == lm.SETUP_LOAD
    assert s3["elimination_used"] == lm.ELIM_CAPTURES
    assert_matches_fresh_load(s2, camera, s3, cam_f)


def test_invalid_elimination_rejected(lm):
    g = synth.config_graph("tiny")
    with pytest.raises(lm.LMError):
        lm.solve_graph(g, elimination=7)
