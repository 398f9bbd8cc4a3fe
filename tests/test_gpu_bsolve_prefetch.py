"""k_bsolve_dag's software-pipelined gather loop against the build before it.  A dense matrix of T
tiles gives column k of the persistent backward solve a gather list of T-1-k items, so small sizes
run every shape of the pipeline (tools/make_bsolve_golden.py lists them): no gather at all and the
rhs row in the column's own tile (n = 63), the rhs row alone in the last tile (64), a partial tile
(100), list lengths 0..3 -- empty, prologue only, one swap of the register sets, steady state (200)
-- and both register sets reused (321).  tests/golden/bsolve_parent.npz holds the y vectors the
parent build computed from the same seeds; the products, the order of summation and the hand-off
are unchanged (only when the loads are issued differs), so y must agree bit for bit.  A sparse
graph then runs gather lists with structurally missing tiles through the plan's stored tile index."""
import os
import sys

import numpy as np
import pytest

from ar_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_bsolve_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    d = np.load(os.path.join(ROOT, "tests", "golden", "bsolve_parent.npz"))
    assert tuple(d["sizes"]) == G.SIZES
    assert list(d["seeds"]) == [G.system(n)[0] for n in G.SIZES]
    return d


@pytest.mark.parametrize("n", G.SIZES)
def test_dense_back_solve_bit_identical_to_parent(lm, golden, n):
    _, A, b = G.system(n)
    y = G.solve(lm, n)
    want = golden[f"y_{n}"]
    r, r_np = G.residual(A, y, b), G.residual(A, np.linalg.solve(A, b), b)
    print(f"n {n}: residual {r:.3e}, numpy.linalg.solve {r_np:.3e}, differing entries {int((y != want).sum())}")
    assert y.tobytes() == want.tobytes()
    # against the math: no worse than twice a float64 LAPACK solve's residual on the same system
    # (slack over a reference of the same precision), or 64 eps where that residual is (near) zero
    assert r <= max(2.0 * r_np, 64 * np.finfo(np.float64).eps)


def test_sparse_pattern_executors_agree(lm):
    """medium (200 captures): the persistent executor (k_bsolve_dag, the stored tile index of every
    gathered tile) against the level launches (k_bs_gather / k_bs_solve, which look the tile up),
    compared as tests/test_gpu_parity.py compares the two executors."""
    g = synth.config_graph("medium")
    out = []
    for ex in (1, 0):
        rp = lm.ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, factor_executor=ex)
        out.append(rp.solve())
    dag, lev = out
    assert dag["termination"] == lev["termination"] and dag["rule"] == lev["rule"]
    assert len(dag["iterations"]) == len(lev["iterations"])
    assert dag["num_linear_solves"] == lev["num_linear_solves"]
    np.testing.assert_allclose([i["cost"] for i in dag["iterations"]], [i["cost"] for i in lev["iterations"]],
                               rtol=1e-10)
    np.testing.assert_allclose(dag["final_cost"], lev["final_cost"], rtol=1e-10)
