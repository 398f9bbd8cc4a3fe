"""What the localizer's covariance costs on the cfg5 batch (debug / profiles/localize_cov).

One process, two resident handles on the 4,096-query cfg5 batch (no loss; Cauchy(3 px)): 3
warm-up rounds, then ROUNDS rounds of solve() + covariance() on each in turn, both timed by the
handle's HIP events around the launch (solve: k_tag_corners + k_localize; covariance:
k_localize_cov).  Prints medians (min - max) and the ratio.

usage: python tools/loc_cov_cost.py [rounds]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ar_slam_amd import lm, synth  # noqa: E402


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    b = synth.make_localize_batch(n_query=4096)
    handles = {"no loss": lm.Localizer(b), "Cauchy(3 px)": lm.Localizer(b, loss=(lm.LOSS_CAUCHY, 3.0))}
    t = {k: ([], []) for k in handles}
    iters, pivots, status = {}, {}, {}
    for r in range(3 + rounds):
        for k, h in handles.items():
            _, res, ms = h.solve()
            cov, st, mp, cms = h.covariance(timed=True)
            if r >= 3:
                t[k][0].append(ms)
                t[k][1].append(cms)
            iters[k], pivots[k], status[k] = int(res["num_iterations"].sum()), mp, st
    print(f"cfg5: {b.n_query} queries x 8 tags, medians of {rounds} (min - max), kernel ms by HIP events")
    print(f"{'':14s}{'solve':>30s}{'covariance':>30s}   ratio   LM iterations   status OK   min_pivot min / median")
    for k in handles:
        s, c = np.array(t[k][0]), np.array(t[k][1])
        ok = status[k] == lm.COV_OK
        print(f"{k:14s}{np.median(s):12.4f} ({s.min():.4f} - {s.max():.4f})"
              f"{np.median(c):12.4f} ({c.min():.4f} - {c.max():.4f})   {np.median(c) / np.median(s):.3f}"
              f"   {iters[k]:13d}   {ok.sum():9d}   {pivots[k][ok].min():.2e} / {np.median(pivots[k][ok]):.2e}")


if __name__ == "__main__":
    main()
