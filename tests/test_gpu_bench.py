"""bench.py's plain and --full runs on a small graph.

A plain run (`--gpus 1 --steps K --warmup W`) times K solves and prints the headline line with
nothing that takes a run of its own; `--dump-outputs DIR` writes what the last timed solve gave
its caller; `--full` adds the per-phase solve, the box fingerprint and the CPU baseline.  The
dumped results are checked against the CPU oracle on the same seeded graph, as smoke() checks a
solve (cost trace to 1e-9)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "small", *args],
                         capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_last_solve(lm, oracle, tmp_path):
    from ar_slam_amd import synth
    d = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out"))
    assert all(k in d for k in HEADLINE), sorted(d)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "LM iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["termination"].startswith("CONVERGENCE"), d["termination"]
    # nothing that takes a run of its own
    assert d["phase_ms_per_solve"] is None and d["cpu_baseline"] is None
    assert not [k for k in d if k.startswith(("box_fingerprint", "incremental_", "localize_", "cpu_baseline_"))]
    g = synth.config_graph("small")
    got = {n: np.load(tmp_path / "out" / f"{n}.npy") for n in ("camera", "cap", "tag", "cost_trace")}
    assert sorted(os.listdir(tmp_path / "out")) == sorted(n + ".npy" for n in got)
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["camera"].shape == (3,) and got["cap"].shape == (g.n_cap, 6) and got["tag"].shape == (g.n_tag, 6)
    _, _, _, ref = oracle.solve_graph(g)
    cr = np.array([it["cost"] for it in ref["iterations"]])
    n = min(len(cr), len(got["cost_trace"]), 5)
    assert n >= 2 and np.all(np.abs(got["cost_trace"][:n] - cr[:n]) <= 1e-9 * np.abs(cr[:n])), (got["cost_trace"], cr)
    # the solved poses, not the initial state
    assert not np.array_equal(got["cap"], g.cap) and not np.array_equal(got["tag"], g.tag)


def test_full_run_adds_the_side_measurements(lm):
    d = _bench("--steps", "2", "--warmup", "1", "--full", "--cpu-threads", "2")
    assert all(k in d for k in HEADLINE), sorted(d)
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert set(d["phase_ms_per_solve"]) == {"linearize", "schur", "cholesky", "solve", "backsub", "cost"}
    assert d["box_fingerprint"]["pingpong_ns"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] == 2
