"""What an anchored covariance call costs under the mixed e-block set (debug / profiles/lm_cov_anchored).

One process, two resident handles on one config (cfg2 by default), interleaved: the problem with no
constant block under ELIM_MIXED and covariance_anchored((BLOCK_TAG, 0)), against the same problem
with tag 0 constant under ELIM_CAPTURES and covariance().  Prints the four device times of each
call (HIP events: linearization, reduced system + factorization, selected inverse, marginal
blocks), medians of ROUNDS rounds after a warm-up, and sigma_f by both (gauge invariant).

usage: python tools/lm_cov_anchored_cost.py [rounds] [config]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ar_slam_amd import lm, synth  # noqa: E402

PHASES = ["t_linearize_ms", "t_factor_ms", "t_selinv_ms", "t_blocks_ms"]


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    name = sys.argv[2] if len(sys.argv) > 2 else "cfg2"
    g = synth.config_graph(name)
    tag_const = np.zeros(g.n_tag, np.uint8)
    tag_const[0] = 1
    args = (g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    mixed = lm.ResidentProblem(*args, elimination=lm.ELIM_MIXED, phase_timing=1)
    caps = lm.ResidentProblem(*args, tag_const=tag_const, elimination=lm.ELIM_CAPTURES, phase_timing=1)
    calls = {"mixed, anchored at tag 0": (mixed, lambda: mixed.covariance_anchored((lm.BLOCK_TAG, 0))),
             "captures, tag 0 constant": (caps, caps.covariance)}
    t = {k: {p: [] for p in PHASES} for k in calls}
    out, used = {}, {}
    for r in range(1 + rounds):
        for k, (rp, call) in calls.items():
            used[k] = rp.solve()["elimination_used"]
            out[k] = call()
            if r:
                for p in PHASES:
                    t[k][p].append(out[k]["info"][p])
    print(f"{name}: {g.n_cap} captures, {g.n_tag} tags, {g.n_obs} observations; medians of {rounds} rounds (min - max), "
          "device ms by HIP events")
    for k in calls:
        info = out[k]["info"]
        print(f"{k}: elimination_used {used[k]}, {info['n_reduced']} reduced rows, {info['n_factor_tiles']} factor tiles, "
              f"status {info['status']}, min_pivot {info['min_pivot']:.3e}")
        total = np.zeros(rounds)
        for p in PHASES:
            v = np.array(t[k][p])
            total += v
            print(f"  {p[2:-3]:10s} {np.median(v):9.3f} ({v.min():.3f} - {v.max():.3f})")
        print(f"  {'total':10s} {np.median(total):9.3f} ({total.min():.3f} - {total.max():.3f})")
    a, b = out["mixed, anchored at tag 0"], out["captures, tag 0 constant"]
    for key in ("cap", "tag"):
        assert np.array_equal(a[key + "_status"], b[key + "_status"])
    # (the pose blocks are not compared: the gauge-free solve ends in another frame than the one
    # with tag 0 held, and a block's coordinates turn with the frame; var(f) does not)
    print(f"sigma_f at 0.5 px: {0.5 * np.sqrt(a['var_f']):.4f} / {0.5 * np.sqrt(b['var_f']):.4f} px")


if __name__ == "__main__":
    main()
