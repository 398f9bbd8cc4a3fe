"""k_schur<false>'s table-driven output stage against the build before it: a graph whose captures
see 1, 2, ..., 11 distinct tags in turn runs every shape of the 16x16-tile output product -- one
tile row (nblk 1, 2: M = 8, 14), the 16-boundaries (nblk 3, 5: M = 20, 32), cfg3's shape (nblk 8,
M = 50), all 13 tiles (nblk 10, M = 62), one capture on the big path (nblk 11) and two observation
chunks (9-11 tags).  tests/golden/schur_k1to11.npz holds the iteration costs and final parameters
the parent build computed on the same graph (tools/make_schur_golden.py); the slab layout, the MFMA
operands and the ff - acc expression are unchanged, so the results must agree bit for bit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_schur_golden as G  # noqa: E402
from test_gpu_parity import _compare_solves  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def graph():
    return G.graph()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "schur_k1to11.npz"))


def _check_golden(ours, golden, tag):
    cam, cap, tg, s = ours
    assert np.array_equal(np.array([i["cost"] for i in s["iterations"]], np.float64), golden[f"{tag}_cost"])
    assert np.array_equal(cam, golden[f"{tag}_camera"])
    assert np.array_equal(cap, golden[f"{tag}_cap"])
    assert np.array_equal(tg, golden[f"{tag}_tag"])


def test_graph_shapes(graph):
    """(no solve) the captures' distinct-tag counts are 1..11 in turn, four times over"""
    n = [len(set(graph.obs_tag[graph.obs_cap == c])) for c in range(graph.n_cap)]
    assert n == [1 + c % 11 for c in range(44)]


def test_k1to11_bit_identical_to_parent_and_matches_oracle(lm, oracle, graph, golden):
    ours = G.solve(graph, const=False)
    assert ours[3]["elimination_used"] == lm.ELIM_CAPTURES
    _check_golden(ours, golden, "free")
    ref = oracle.solve_graph(graph)
    assert ref[3]["termination"] == "CONVERGENCE"
    _compare_solves(graph, ours, ref)


def test_k1to11_constant_tag_and_camera(lm, oracle, graph, golden):
    """One tag and the camera constant: a second kind of block per capture, whose entries are stored
    but never gathered."""
    ours = G.solve(graph, const=True)
    _check_golden(ours, golden, "const")
    cc, tc = G.const_blocks(graph)
    ref = oracle.solve(graph.camera, graph.cap, graph.tag, graph.obs_cap, graph.obs_tag, graph.corners,
                       camera_const=cc, tag_const=tc)
    _compare_solves(graph, ours, ref)
