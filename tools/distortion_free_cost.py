"""What estimating the distortion costs on the device (debug / profiles/distortion_free).

cfg3 generated through the lens l = (-0.12, 0.03), solved under CAMERA_RADIAL twice: with the
lens known (l1, l2 held: the kDist instances, tools/distortion_cost.py's "radial" side) and with
estimate_distortion on from l = (0, 0) (k_linearize_est, k_cam_l_reduce + k_slot_norms_l,
k_schur_cam + k_schur_cam_gather after k_schur's own gather, k_backsub_est), interleaved over
ROUNDS rounds on two resident handles.  Per phase, the summary's device time (HIP events around
the phases) divided by the solve's linear solves, medians over the rounds, the difference and
the ratio.  The Schur phase is k_schur + its gather on the known side and the same plus the
border's two kernels on the estimated side, so its difference is what the border costs.

The two solves start from different lenses, so their iteration counts can differ: every figure
is per linear solve.

usage: python tools/distortion_free_cost.py [rounds] [config]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ar_slam_amd import lm, synth  # noqa: E402

PHASES = ["t_linearize_ms", "t_schur_ms", "t_cholesky_ms", "t_solve_ms", "t_backsub_ms", "t_cost_ms"]
LENS = (-0.12, 0.03)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    name = sys.argv[2] if len(sys.argv) > 2 else "cfg3"
    lm.warm_up()
    g = synth.config_graph(name, distortion=LENS)
    rest = (g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    cam0 = np.array([g.camera[0], 0.0, 0.0])
    handles = {"known": lm.ResidentProblem(g.camera, *rest, camera_model=lm.CAMERA_RADIAL, phase_timing=1),
               "estimated": lm.ResidentProblem(cam0, *rest, camera_model=lm.CAMERA_RADIAL, estimate_distortion=True,
                                               phase_timing=1)}
    per_it = {k: {p: [] for p in PHASES} for k in handles}
    info = {}
    for r in range(1 + rounds):
        for k, rp in handles.items():
            s = rp.solve()
            if r == 0:
                continue
            info[k] = {"linear_solves": s["num_linear_solves"], "termination": s["termination"],
                       "final_rms_px": round(s["final_rms_px"], 4), "camera": [round(float(v), 5) for v in rp.camera]}
            for p in PHASES:
                per_it[k][p].append(s[p] / max(s["num_linear_solves"], 1))
    out = {"config": name, "rounds": rounds, "lens": LENS, "solves": info}
    tot = {"known": 0.0, "estimated": 0.0}
    for p in PHASES:
        d, z = float(np.median(per_it["known"][p])), float(np.median(per_it["estimated"][p]))
        tot["known"] += d
        tot["estimated"] += z
        out[p] = {"known_us_per_iteration": round(1e3 * d, 3), "estimated_us_per_iteration": round(1e3 * z, 3),
                  "difference_us": round(1e3 * (z - d), 3), "ratio": round(z / d, 4) if d > 0 else None}
        print(f"{name} {p[2:-3]:10s} known {1e3 * d:8.2f} us / iteration   estimated {1e3 * z:8.2f} us   "
              f"difference {1e3 * (z - d):+8.2f} us   ratio {z / d if d > 0 else float('nan'):.3f}")
    print(f"{name} {'all phases':10s} known {1e3 * tot['known']:8.2f} us / iteration   estimated "
          f"{1e3 * tot['estimated']:8.2f} us   difference {1e3 * (tot['estimated'] - tot['known']):+8.2f} us   "
          f"ratio {tot['estimated'] / tot['known']:.3f}")
    for k, v in info.items():
        print(f"{name} {k}: {v['linear_solves']} linear solves, {v['termination']}, RMS {v['final_rms_px']} px, "
              f"camera {v['camera']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
