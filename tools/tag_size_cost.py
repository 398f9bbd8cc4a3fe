"""What per-tag side lengths cost on the device (debug / profiles/tag_size).

cfg3 with every tag's side set to a non-default value (uniform 0.10 m: the sized instances of
k_linearize, k_backsub and the candidate cost) against the same problem without sizes (the
default instances), interleaved over ROUNDS rounds on two resident handles: the per-solve device
times t_linearize_ms, t_backsub_ms and t_cost_ms of the summary (phase timers) divided by the
solve's linear solves, and their ratios.  Then a cfg5 batch (4096 queries) with tag_size given
against the same batch without: the solve's kernel time (k_tag_corners + k_localize).

The sized problems are the default ones in another unit (every translation times 0.10 / 0.0635),
so both sides see the same scene and run the same iterations.

usage: python tools/tag_size_cost.py [rounds] [config]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ar_slam_amd import lm, synth  # noqa: E402

PHASES = ["t_linearize_ms", "t_backsub_ms", "t_cost_ms"]


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    name = sys.argv[2] if len(sys.argv) > 2 else "cfg3"
    g = synth.config_graph(name)
    lm.warm_up()
    arrays = (g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    # (the translations scaled with the side: the same scene in the sized problem's unit, so both
    # handles run the same number of iterations on equally good starts)
    lam = 0.10 / lm.DEFAULT_TAG_SIZE
    cap, tag = g.cap.copy(), g.tag.copy()
    cap[:, :3] *= lam
    tag[:, :3] *= lam
    handles = {"default": lm.ResidentProblem(*arrays, phase_timing=1),
               "sized": lm.ResidentProblem(g.camera, cap, tag, g.obs_cap, g.obs_tag, g.corners, tag_size=0.10,
                                           phase_timing=1)}
    per_it = {k: {p: [] for p in PHASES} for k in handles}
    iters = {}
    for r in range(1 + rounds):
        for k, rp in handles.items():
            s = rp.solve()
            if r == 0:
                continue
            iters[k] = s["num_linear_solves"]
            for p in PHASES:
                per_it[k][p].append(s[p] / max(s["num_linear_solves"], 1))
    out = {"config": name, "rounds": rounds, "linear_solves": iters}
    for p in PHASES:
        d, z = np.median(per_it["default"][p]), np.median(per_it["sized"][p])
        out[p] = {"default_us_per_iteration": round(1e3 * d, 3), "sized_us_per_iteration": round(1e3 * z, 3),
                  "ratio": round(float(z / d), 4) if d > 0 else None}
        print(f"{name} {p[2:-3]:10s} default {1e3 * d:8.2f} us / iteration   sized {1e3 * z:8.2f} us   ratio {z / d if d > 0 else float('nan'):.3f}")
    b = synth.make_localize_batch(n_query=4096)
    import dataclasses
    big = b.tag.copy()
    big[:, :3] *= lam   # (the same map in the sized batch's unit: the same queries, lam times farther away)
    locs = {"default": lm.Localizer(b), "sized": lm.Localizer(dataclasses.replace(b, tag=big), tag_size=0.10)}
    ms = {k: [] for k in locs}
    for r in range(1 + rounds):
        for k, loc in locs.items():
            _, _, t = loc.solve(download=False)
            if r:
                ms[k].append(t)
    d, z = np.median(ms["default"]), np.median(ms["sized"])
    out["cfg5_kernel_ms"] = {"default": round(float(d), 4), "sized": round(float(z), 4)}
    print(f"cfg5 4096 queries: default {d:.4f} ms   with tag_size {z:.4f} ms   ratio {z / d:.3f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
