"""What the radial camera model costs on the device (debug / profiles/distortion).

cfg3 generated through the lens l = (-0.12, 0.03) and solved under CAMERA_RADIAL (the kDist
instances of k_linearize, k_backsub and the candidate cost) against the same graph generated
without a lens and solved under CAMERA_PINHOLE (the instances every problem ran before: their
machine code is the parent's, profiles/distortion/isa_unchanged.txt), interleaved over ROUNDS
rounds on two resident handles: the per-solve device times t_linearize_ms, t_backsub_ms and
t_cost_ms of the summary (HIP events around the phases) divided by the solve's linear solves,
medians over the rounds, and their ratios.  Then the cfg5 batch (4096 queries) both ways: the
solve's kernel time (k_tag_corners + k_localize), per query and per LM iteration.

The two sides see the same cameras and tags; the lens moves the detections (and, through the
visibility test, a few of the tags a capture sees), so the iteration counts can differ by one:
the mapper's figures are per linear solve, the localizer's also per iteration.

usage: python tools/distortion_cost.py [rounds] [config]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ar_slam_amd import lm, synth  # noqa: E402

PHASES = ["t_linearize_ms", "t_backsub_ms", "t_cost_ms"]
LENS = (-0.12, 0.03)


def _arrays(g):
    return (g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    name = sys.argv[2] if len(sys.argv) > 2 else "cfg3"
    lm.warm_up()
    handles = {"pinhole": lm.ResidentProblem(*_arrays(synth.config_graph(name)), phase_timing=1),
               "radial": lm.ResidentProblem(*_arrays(synth.config_graph(name, distortion=LENS)),
                                            camera_model=lm.CAMERA_RADIAL, phase_timing=1)}
    per_it = {k: {p: [] for p in PHASES} for k in handles}
    iters, term = {}, {}
    for r in range(1 + rounds):
        for k, rp in handles.items():
            s = rp.solve()
            if r == 0:
                continue
            iters[k] = s["num_linear_solves"]
            term[k] = s["termination"]
            for p in PHASES:
                per_it[k][p].append(s[p] / max(s["num_linear_solves"], 1))
    out = {"config": name, "rounds": rounds, "lens": LENS, "linear_solves": iters, "termination": term}
    for p in PHASES:
        d, z = np.median(per_it["pinhole"][p]), np.median(per_it["radial"][p])
        out[p] = {"pinhole_us_per_iteration": round(1e3 * d, 3), "radial_us_per_iteration": round(1e3 * z, 3),
                  "ratio": round(float(z / d), 4) if d > 0 else None}
        print(f"{name} {p[2:-3]:10s} pinhole {1e3 * d:8.2f} us / iteration   radial {1e3 * z:8.2f} us   "
              f"ratio {z / d if d > 0 else float('nan'):.3f}")
    locs = {"pinhole": lm.Localizer(synth.make_localize_batch(n_query=4096)),
            "radial": lm.Localizer(synth.make_localize_batch(n_query=4096, distortion=LENS),
                                   camera_model=lm.CAMERA_RADIAL)}
    ms = {k: [] for k in locs}
    its = {}
    for r in range(1 + rounds):
        for k, loc in locs.items():
            if r == 0:
                _, res, _ = loc.solve()
                its[k] = float(np.mean(res["num_iterations"]))
                continue
            _, _, t = loc.solve(download=False)
            ms[k].append(t)
    d, z = np.median(ms["pinhole"]), np.median(ms["radial"])
    out["cfg5_kernel_ms"] = {"pinhole": round(float(d), 4), "radial": round(float(z), 4),
                             "ratio": round(float(z / d), 4),
                             "mean_iterations": {k: round(v, 3) for k, v in its.items()},
                             "ratio_per_iteration": round(float((z / its["radial"]) / (d / its["pinhole"])), 4)}
    print(f"cfg5 4096 queries: pinhole {d:.4f} ms ({its['pinhole']:.2f} iterations / query)   radial {z:.4f} ms "
          f"({its['radial']:.2f})   ratio {z / d:.3f}, per iteration {(z / its['radial']) / (d / its['pinhole']):.3f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
