"""What arslam_lm_evaluate costs on the device (debug / profiles/evaluate).

One resident handle of a config (cfg3), phase_timing = 1: HIP events on the handle's stream around
the parameter upload, each of the evaluate path's kernels and the copy back
(arslam_lm_debug_evaluate_times), after warm-up calls, medians of REPS calls -- with and without
the residuals (8 doubles per observation more to store and to copy back), and with a Cauchy loss.
Beside them, as the yardstick, the linearization phase of one LM iteration of the same handle:
summary.t_linearize_ms of a solve of no iterations (k_linearize, its reductions and the slot
norms: the solver's own evaluation of the same rows, unchanged by the evaluate path).

The bytes are algorithmic, counted here per observation (what the kernel must read and write once,
whatever the caches do), and the rate they give is set against the MI355X's measured HBM peak.

usage: python tools/evaluate_cost.py [reps] [config]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ar_slam_amd import lm, synth  # noqa: E402

HBM_PEAK = 6.29e12   # B/s, measured float4 copy (8.0e12 spec)
PHASES = ("upload", "k_eval_obs", "k_eval_blocks", "k_eval_tree", "copy_back")


def obs_bytes(residuals, loss):
    """k_eval_obs per observation: indices 8, corners 64, the camera, capture and tag values it
    gathers 24 + 48 + 48, the loss's kind and scale 9; stores 18 items of 8, and the 8 residuals."""
    return 8 + 64 + 120 + (9 if loss else 0) + 18 * 8 + (64 if residuals else 0)


BLOCKS_BYTES = 12 * 8 + 2 * 4   # k_eval_blocks per observation: its 12 pose contributions, its two list entries
TREE_BYTES = 4 * 8              # k_eval_tree per observation: f, l1, l2 contributions and rho


def measure(rp, reps, **kw):
    for _ in range(2):
        rp.evaluate(**kw)
    rows, wall = [], []
    for _ in range(reps):
        t = time.perf_counter()
        rp.evaluate(**kw)
        wall.append(time.perf_counter() - t)
        rows.append(rp.debug_evaluate_times())
    med = {p: float(np.median([r[p] for r in rows])) for p in PHASES}
    med["wall"] = 1e3 * float(np.median(wall))
    return med


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    name = sys.argv[2] if len(sys.argv) > 2 else "cfg3"
    lm.warm_up()
    g = synth.config_graph(name)
    arrays = (g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    nb, n = g.n_obs, 3 + 6 * g.n_cap + 6 * g.n_tag
    out = {"config": name, "reps": reps, "n_obs": nb, "n_params": n, "hbm_peak_Bps": HBM_PEAK}
    print(f"{name}: {nb} observations, {g.n_cap} captures, {g.n_tag} tags, {n} parameters; medians of {reps}")
    for label, loss in (("no loss", None), ("cauchy(3)", (lm.LOSS_CAUCHY, 3.0))):
        rp = lm.ResidentProblem(*arrays, loss=loss, phase_timing=1, max_num_iterations=0)
        # the yardstick: one linearization of the solver (a solve of no iterations)
        lin = []
        for r in range(2 + reps):
            s = rp.solve()
            if r >= 2:
                lin.append(s["t_linearize_ms"])
        lin_ms = float(np.median(lin))
        print(f"{name} {label}: solver linearization phase (k_linearize + reductions + norms, "
              f"{len(s['iterations'])} iteration record) {1e3 * lin_ms:8.2f} us")
        out[label] = {"solver_linearize_us": round(1e3 * lin_ms, 3)}
        for res in (True, False):
            m = measure(rp, reps, residuals=res)
            key = "with residuals" if res else "without residuals"
            b_obs, b_blk, b_tree = obs_bytes(res, loss is not None) * nb, BLOCKS_BYTES * nb, TREE_BYTES * nb
            rate = b_obs / (1e-3 * m["k_eval_obs"]) if m["k_eval_obs"] > 0 else 0.0
            dev = sum(m[p] for p in PHASES)
            back = 8 * (1 + n + 2 * nb + (8 * nb if res else 0))
            print(f"{name} {label} {key}: upload {1e3 * m['upload']:7.2f} us ({8 * n} B)  k_eval_obs "
                  f"{1e3 * m['k_eval_obs']:7.2f} us ({b_obs} B, {rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of "
                  f"the HBM peak)  k_eval_blocks {1e3 * m['k_eval_blocks']:7.2f} us ({b_blk} B, "
                  f"{b_blk / (1e-3 * m['k_eval_blocks']) / 1e12 if m['k_eval_blocks'] > 0 else 0:.3f} TB/s)  k_eval_tree x2 "
                  f"{1e3 * m['k_eval_tree']:7.2f} us ({b_tree} B)  copy back {1e3 * m['copy_back']:8.2f} us ({back} B)  "
                  f"device total {1e3 * dev:8.2f} us  call wall {1e3 * m['wall']:8.2f} us  "
                  f"kernels / solver linearization {(m['k_eval_obs'] + m['k_eval_blocks'] + m['k_eval_tree']) / lin_ms:.3f}")
            out[label][key] = {**{p + "_us": round(1e3 * m[p], 3) for p in PHASES}, "wall_us": round(1e3 * m["wall"], 3),
                               "k_eval_obs_bytes": b_obs, "k_eval_obs_Bps": round(rate, 0),
                               "k_eval_obs_fraction_of_hbm_peak": round(rate / HBM_PEAK, 4),
                               "k_eval_blocks_bytes": b_blk, "k_eval_tree_bytes": b_tree, "copy_back_bytes": back}
        rp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
