"""GPU tests of the Cholesky chain's hand-offs in k_factor_dag: the solved tile stored by the wave
that solved each row block, and the root column's inverse formed by its POTRF task from LDS (no
INV task for it, tests/test_chain_handoff_plan.py).  Both move work that already existed, so every
result is compared bit for bit:

  * the persistent executor against the level-launch executor (factor_executor 0), on whole LM
    solves and on the factorization alone (arslam_debug_tile_llt: the factor's tiles, and the
    solution y, which the backward solve forms with every column's inverse tile, the root's first
    -- no debug entry returns the inverse tiles themselves);
  * few-workgroup grids (arslam_debug_dag_workgroup_limit 1, 2, 7) against the full grid;
  * a forced multi-rank solve (two-phase plan: only the last column of the last phase is the root)
    against the plain solve, pose for pose as tests/test_gpu_multirank.py holds cfg2.

Shapes: `tiny` has two tile columns, the tile inputs dense_n1 / dense_n63 one (the root POTRF is
then drawn, not continued, and is the launch's only POTRF) and dense_n65 two; `medium` (9 columns)
and nd12 (12) are the smallest plans with merges, continuations and fused tiles.

The two executors' backward solves sum a column's gathered terms L_ik^T y_i in the same order (the
level launches took k_bsolve_dag's: a wave's rows into one accumulator, the nearest ancestor last;
they used to sum two accumulators per wave and the nearest ancestor first, and then `medium`'s
traces agreed to 8e-14 and nd12's y to 2.8e-13 only), so whole solves agree bit for bit.
"""
import numpy as np
import pytest

import llt_ref as R
from gauge import assert_poses_match

pytestmark = pytest.mark.gpu

SHAPES = ["tiny", "medium"]
TILE_INPUTS = ["dense_n1", "dense_n63", "dense_n65", "nd12_n740_c8"]


@pytest.fixture(scope="module")
def lm():
    from ar_slam_amd import build, lm as _lm
    build.build()
    return _lm


def _part(name):
    from ar_slam_amd import synth
    g = synth.config_graph(name)
    return dict(camera=g.camera, cap=g.cap, tag=g.tag, obs_cap=g.obs_cap, obs_tag=g.obs_tag, corners=g.corners)


def _solve(lm, name, **kw):
    rp = lm.ResidentProblem(**_part(name), **kw)
    try:
        s = rp.solve()
        return dict(cost=[it["cost"] for it in s["iterations"]], camera=rp.camera.copy(), cap=rp.cap.copy(),
                    tag=rp.tag.copy(), termination=s["termination"], rule=s["rule"])
    finally:
        rp.close()


_full_grid = {}


def _persistent(lm, name):
    """The persistent executor's solve on the full grid: computed once, shared, left unchanged."""
    if name not in _full_grid:
        _full_grid[name] = _solve(lm, name, factor_executor=1)
    return _full_grid[name]


def _assert_same_solve(a, b, what):
    assert a["cost"] == b["cost"], (what, a["cost"], b["cost"])
    assert (a["termination"], a["rule"]) == (b["termination"], b["rule"]), what
    for k in ("camera", "cap", "tag"):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("name", SHAPES)
def test_persistent_executor_equals_level_launches(lm, name):
    dag, lev = _persistent(lm, name), _solve(lm, name, factor_executor=0)
    print(f"chain_handoff: {name} cost trace, persistent {dag['cost']} level launches {lev['cost']}")
    assert len(dag["cost"]) > 1
    _assert_same_solve(dag, lev, name)


@pytest.mark.parametrize("name", TILE_INPUTS)
def test_factor_and_root_inverse_equal_the_level_launches(lm, name):
    inp = R.make_input(name)
    L1, y1, info1, pat1, facts = lm.debug_tile_llt(inp.A, inp.b, inp.pattern, executor=1)
    L0, y0, info0, pat0, _ = lm.debug_tile_llt(inp.A, inp.b, inp.pattern, executor=0)
    print(f"chain_handoff: {name} tasks {facts['n_dag_tasks']} max |L1 - L0| {np.max(np.abs(L1 - L0)):.3e} "
          f"max |y1 - y0| {np.max(np.abs(y1 - y0)):.3e}")
    assert info1 == 0 and info0 == 0
    assert np.array_equal(pat1, pat0)
    assert np.all(np.isfinite(L1)) and np.all(np.isfinite(y1))
    assert L1.tobytes() == L0.tobytes()
    # y: the backward solve forms it with every column's inverse tile, the root's first (its rows
    # have no gathered term); both executors sum a column's gathered terms in the same order
    assert y1.tobytes() == y0.tobytes()


@pytest.mark.parametrize("k", [1, 2, 7])
def test_few_workgroup_grids_solve_the_same_bits(lm, k):
    full = _persistent(lm, "medium")
    lm.debug_dag_workgroup_limit(k)
    try:
        few = _solve(lm, "medium", factor_executor=1)
    finally:
        lm.debug_dag_workgroup_limit(0)
    _assert_same_solve(full, few, f"{k} workgroups")


def test_forced_multirank_solve_matches_the_plain_solve(lm):
    """One rank on the two-rank split's plan through the callback transport (the all-reduce of one
    rank is the identity): the two-phase factorization sums a top tile's updates subtree-first, so
    the last bits may differ from the plain solve; the poses match (tests/test_gpu_multirank.py's
    bounds for cfg2)."""
    plain = _persistent(lm, "medium")
    rp = lm.ResidentProblem(**_part("medium"), comm=(0, 1, lambda a, op: None), force_multirank=True,
                            factor_executor=1)
    try:
        s = rp.solve()
        cost = [it["cost"] for it in s["iterations"]]
        cam, cap, tag = rp.camera.copy(), rp.cap.copy(), rp.tag.copy()
    finally:
        rp.close()
    assert s["n_top_tiles"] > 0 and s["comm_calls"] > 0   # the multi-rank path ran
    assert (s["termination"], s["rule"]) == (plain["termination"], plain["rule"])
    assert len(cost) == len(plain["cost"])
    for a, b in zip(cost, plain["cost"]):
        assert abs(a - b) <= 1e-9 * abs(b), (cost, plain["cost"])
    assert abs(cam[0] - plain["camera"][0]) <= 1e-8 * plain["camera"][0]
    assert_poses_match(cap, tag, plain["cap"], plain["tag"])
