"""CPU test of the backward solve's plan-side tile index: k_bsolve_dag reads the compact index of a
gathered tile (i, k) from the plan's list instead of looking it up in the T x T tile map, so every
entry of that list must be the map's entry of its tile, and a tile of the factor.  The lists come
from the plan dump arslam_debug_reduced_plan writes under ARSLAM_DAG_DUMP (tools/dag_dump.py)."""
import os
import sys

import numpy as np
import pytest

from ar_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dag_dump  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from ar_slam_amd import build, lm
    build.build()
    return lm


@pytest.mark.parametrize("name", ["tiny", "medium", "cfg2"])
def test_gather_entries_carry_their_tile_index(L, name, tmp_path, monkeypatch):
    g = synth.config_graph(name)
    path = tmp_path / "plan.bin"
    monkeypatch.setenv("ARSLAM_DAG_DUMP", str(path))
    info, _ = L.debug_reduced_plan(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    d = dag_dump.load(str(path))
    T = d["T"]
    assert T == info["tiles_per_side"]
    gather, gtile = d["gather"], d["gtile"]
    assert len(gather) == len(gtile)
    # one entry per below-diagonal tile of the factor: every column is gathered on one rank
    assert len(gather) == info["n_factor_tiles"] - T
    if name != "tiny":
        assert len(gather) > 0
    i, k = gather[:, 0], gather[:, 1]
    assert ((0 <= k) & (k < i) & (i < T)).all()
    np.testing.assert_array_equal(gtile, d["tmap"][i, k])
    assert (gtile >= 0).all() and (gtile < info["n_factor_tiles"]).all()
    assert len(set(zip(i.tolist(), k.tolist()))) == len(gather)   # each tile once
