"""GPU tests of the chain POTRF's side work in k_factor_dag: waves 1-3 count their update round before
the caller's side work (the fused tile's fetch, the counter polls, the continuation's record, the
fused solve's early steps) instead of after it, so wave 0 no longer waits for work it does not need
(blocked_potrf64_async, kPfCountFirst).  Only when things happen changes -- the products and their
order are the same -- so every result is compared bit for bit:

  * dense systems of 1 to 6 tile columns (the sizes of tools/make_bsolve_golden.py: n = 63 no fused
    tile; 64 and 100 one fused tile with its continuation; 200 and 321 fused tiles whose last update
    arrives during the POTRF): the persistent executor's factor and y against the level launches',
    which run the barrier POTRF -- the same products, none of this scheduling;
  * the same systems with only 1, 2 or 7 workgroups started (at 1 every fused tile is ready before
    panel 0 and its fetch starts beside panel 1; at 2 and 7 it arrives late and the fetch falls
    beside panels 2 and 3 or after the publish) against the full grid;
  * `medium` (200 captures): the persistent executor's LM cost trace and final parameters against
    tests/golden/potrf_sidework_parent.npz, recorded from the build before this change by
    tools/make_potrf_sidework_golden.py.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_bsolve_golden as G  # noqa: E402
import make_potrf_sidework_golden as P  # noqa: E402

pytestmark = pytest.mark.gpu

LIMITS = [1, 2, 7]

_full_grid = {}


def _factor(lm, n, executor):
    _, A, b = G.system(n)
    L, y, info, pat, facts = lm.debug_tile_llt(A, b, None, executor=executor)
    assert info == 0, (n, executor, info)
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(y))
    return L, y, pat, facts


def _persistent(lm, n):
    """The persistent executor's factor and y on the full grid: computed once, shared, left unchanged."""
    if n not in _full_grid:
        _full_grid[n] = _factor(lm, n, 1)
    return _full_grid[n]


@pytest.mark.parametrize("n", G.SIZES)
def test_dense_factor_equals_the_level_launches(lm, n):
    L1, y1, pat1, facts = _persistent(lm, n)
    L0, y0, pat0, _ = _factor(lm, n, 0)
    print(f"potrf_sidework: n {n} tiles/side {facts['tiles_per_side']} tasks {facts['n_dag_tasks']} "
          f"continuations {facts['n_cont_tasks']} max |L1 - L0| {np.max(np.abs(L1 - L0)):.3e} "
          f"max |y1 - y0| {np.max(np.abs(y1 - y0)):.3e}")
    assert facts["tiles_per_side"] == (n + 1 + 63) // 64
    assert np.array_equal(pat1, pat0)
    assert L1.tobytes() == L0.tobytes()
    assert y1.tobytes() == y0.tobytes()


@pytest.mark.parametrize("k", LIMITS)
@pytest.mark.parametrize("n", G.SIZES)
def test_dense_factor_on_few_workgroups_equals_the_full_grid(lm, n, k):
    L1, y1, pat1, _ = _persistent(lm, n)
    lm.debug_dag_workgroup_limit(k)
    try:
        Lk, yk, patk, _ = _factor(lm, n, 1)
    finally:
        lm.debug_dag_workgroup_limit(0)
    print(f"potrf_sidework: n {n}, {k} workgroups: differing entries L {int((Lk != L1).sum())} y {int((yk != y1).sum())}")
    assert np.array_equal(patk, pat1)
    assert Lk.tobytes() == L1.tobytes()
    assert yk.tobytes() == y1.tobytes()


def test_medium_solve_equals_the_parent_build(lm):
    want = np.load(os.path.join(ROOT, "tests", "golden", "potrf_sidework_parent.npz"))
    assert str(want["graph"]) == P.GRAPH
    got = P.solve(lm)
    print(f"potrf_sidework: {P.GRAPH} cost trace {got['cost']} recorded {want['cost']}")
    assert len(got["cost"]) > 1
    assert (str(got["termination"]), str(got["rule"])) == (str(want["termination"]), str(want["rule"]))
    assert int(got["num_linear_solves"]) == int(want["num_linear_solves"])
    assert got["cost"].tobytes() == want["cost"].tobytes()
    for key in ("camera", "cap", "tag"):
        assert got[key].shape == want[key].shape, key
        assert got[key].tobytes() == want[key].tobytes(), key
