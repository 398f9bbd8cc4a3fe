"""CPU tests of the task graph's INV tasks (arslam_debug_dag_tasks): the root column -- the last tile
column, when its POTRF ends the last phase -- has no INV task, because its POTRF task inverts the
L_kk it still holds in LDS (k_factor_dag, kRecInv); every other factored column keeps exactly one,
in its POTRF's phase.  Of a two-rank plan only the true root qualifies: the last column of phase 0
is not the root, the replicated top is factored on every rank.  The protocol simulation
(dag_simulate behind arslam_debug_reduced_plan / arslam_debug_rank_split: every policy, grids of
1..512 workgroups, and 448-workgroup grids of which only 1, 2, 7 or 64 ever start) still finishes
on these plans.
"""
import numpy as np
import pytest

from ar_slam_amd import synth

POTRF, INV = 0, 3
PLANS = [("tiny", 1, 0), ("medium", 1, 0), ("cfg2", 1, 0), ("medium", 2, 0), ("medium", 2, 1)]


@pytest.fixture(scope="module")
def L():
    from ar_slam_amd import build, lm
    build.build()
    return lm


@pytest.mark.parametrize("name,nranks,rank", PLANS)
def test_only_the_root_column_has_no_inv_task(L, name, nranks, rank):
    g = synth.config_graph(name)
    d = L.debug_dag_tasks(g, nranks, rank)
    t, ph = d["tasks"], d["phase"]
    T, last_phase = d["T"], d["n_phases"] - 1
    assert d["n_phases"] == (2 if nranks > 1 else 1)
    potrf = {int(k): int(p) for k, p in zip(t[t[:, 0] == POTRF][:, 1], ph[t[:, 0] == POTRF])}
    assert len(potrf) == int(np.sum(t[:, 0] == POTRF))       # one POTRF per factored column
    inv_cols = t[t[:, 0] == INV][:, 1]
    # the root: the last tile column, factored in the last phase (on every rank of a split)
    assert potrf.get(T - 1) == last_phase
    assert d["root_inv_col"] == T - 1
    assert not np.any(inv_cols == T - 1)
    # every other factored column: exactly one INV task, in its POTRF's phase
    for k, p in potrf.items():
        if k == T - 1:
            continue
        sel = (t[:, 0] == INV) & (t[:, 1] == k)
        assert int(sel.sum()) == 1, (k, int(sel.sum()))
        assert int(ph[sel][0]) == p, (k, int(ph[sel][0]), p)
    assert set(int(k) for k in inv_cols) <= set(potrf)
    if nranks > 1:
        # phase 0 is this rank's subtrees: its last column is not the root and keeps its INV task
        own = [k for k, p in potrf.items() if p == 0]
        assert own and max(own) < T - 1
        assert all(np.any(inv_cols == k) for k in own)
        # tickets [0, phase_split) are phase 0
        assert np.all(ph[:d["phase_split"]] == 0) and np.all(ph[d["phase_split"]:] == 1)


@pytest.mark.parametrize("name,nranks,rank", PLANS)
def test_simulated_interleavings_finish(L, name, nranks, rank):
    g = synth.config_graph(name)
    if nranks == 1:
        info, _ = L.debug_reduced_plan(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    else:
        info, _ = L.debug_rank_split(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, nranks, rank)
    assert info["n_dag_tasks"] == len(L.debug_dag_tasks(g, nranks, rank)["tasks"])
    assert info["dag_valid"] == 1, info   # (negative: -(grid * 16 + policy) of the first deadlock)
