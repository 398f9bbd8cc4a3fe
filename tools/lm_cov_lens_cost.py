"""What the covariance costs with the lens estimated, on cfg3 (debug / profiles/lm_cov_lens).

cfg3's detections through the lens l = (-0.12, 0.03), tag 0 held constant (the anchor).  One
process, two resident handles under CAMERA_RADIAL: `known` holds the true lens and calls
covariance(); `free` starts at l = (0, 0) with estimate_distortion on and calls covariance_lens().
A warm-up round, then ROUNDS rounds, the two handles' calls interleaved (known, free, known, ...)
so both see the same clocks.  Prints the four device times of each call (HIP events, from info:
linearization, reduced system + factorization -- the border kernel and its gather are in this one
--, selected inverse, marginal blocks), their totals and the ratio; then the same for
covariance_pairs() against covariance_pairs_lens() on 100 pairs, the camera in every tenth.
Medians of ROUNDS (min - max).  With an output path the report is also written there.

usage: python tools/lm_cov_lens_cost.py [rounds] [config] [output file]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ar_slam_amd import lm, synth  # noqa: E402

PHASES = ["t_linearize_ms", "t_factor_ms", "t_selinv_ms", "t_blocks_ms"]
LENS = (-0.12, 0.03)


def report(out, label, t):
    total = np.zeros(len(t[PHASES[0]]))
    line = []
    for p in PHASES:
        v = np.array(t[p])
        total += v
        line.append(f"{p[2:-3]} {np.median(v):.3f} ({v.min():.3f} - {v.max():.3f})")
    out(f"  {label:22s} " + "; ".join(line))
    out(f"  {'':22s} total {np.median(total):.3f} ({total.min():.3f} - {total.max():.3f})")
    return float(np.median(total))


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    name = sys.argv[2] if len(sys.argv) > 2 else "cfg3"
    lines = []

    def out(s):
        print(s)
        lines.append(s)

    g = synth.config_graph(name, distortion=LENS)
    tc = np.zeros(g.n_tag, np.uint8)
    tc[0] = 1
    cam0 = g.camera.copy()
    cam0[1:] = 0.0
    known = lm.ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, tag_const=tc,
                               camera_model=lm.CAMERA_RADIAL)
    free = lm.ResidentProblem(cam0, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, tag_const=tc,
                              camera_model=lm.CAMERA_RADIAL, estimate_distortion=True)
    sk, sf = known.solve(), free.solve()
    tk, tf = ({p: [] for p in PHASES} for _ in range(2))
    for r in range(1 + rounds):
        a = known.covariance()
        b = free.covariance_lens()
        if r == 0:
            continue
        for p in PHASES:
            tk[p].append(a["info"][p])
            tf[p].append(b["info"][p])
    assert a["info"]["status"] == lm.COV_OK and b["info"]["status"] == lm.COV_OK
    out(f"{name} through l = {LENS}: {g.n_cap} captures, {g.n_tag} tags, {g.n_obs} observations, tag 0 constant; "
        f"elimination {sf['elimination_used']}, {b['info']['n_reduced']} reduced rows, {b['info']['n_factor_tiles']} factor tiles")
    out(f"known lens: {len(sk['iterations'])} iterations, f = {known.camera[0]:.3f}; estimated from l = (0, 0): "
        f"{len(sf['iterations'])} iterations, f = {free.camera[0]:.3f}, l1 = {free.camera[1]:.5f}, l2 = {free.camera[2]:.5f}")
    sd = 0.5 * np.sqrt(np.diag(b["cam"]))
    out(f"at 0.5 px: 1-sigma f {sd[0]:.4f} px (known lens {0.5 * np.sqrt(a['var_f']):.4f}), l1 {sd[1]:.6f}, l2 {sd[2]:.6f}, "
        f"corr(l1, l2) {b['cam'][1, 2] / np.sqrt(b['cam'][1, 1] * b['cam'][2, 2]):.3f}; min_pivot {b['info']['min_pivot']:.3e} "
        f"(known lens {a['info']['min_pivot']:.3e})")
    out(f"marginals, medians of {rounds} interleaved rounds (min - max), device ms by HIP events")
    mk = report(out, "covariance(), known", tk)
    mf = report(out, "covariance_lens(), free", tf)
    out(f"  the lens costs {mf - mk:+.3f} ms, {mf / mk:.3f} of the known-lens call")
    ok = np.nonzero(b["tag_status"] == lm.COV_OK)[0]
    cam = (lm.BLOCK_CAMERA, 0)
    pairs = [(cam, (lm.BLOCK_TAG, int(ok[2 * k]))) if k % 10 == 0 else
             ((lm.BLOCK_TAG, int(ok[2 * k])), (lm.BLOCK_TAG, int(ok[2 * k + 1]))) for k in range(100)]
    tk, tf = ({p: [] for p in PHASES} for _ in range(2))
    for r in range(1 + rounds):
        _, sa, ia = known.covariance_pairs(pairs)
        _, sb, ib = free.covariance_pairs_lens(pairs)
        assert np.all(sa == lm.COV_OK) and np.all(sb == lm.COV_OK)
        if r == 0:
            continue
        for p in PHASES:
            tk[p].append(ia[p])
            tf[p].append(ib[p])
    out(f"100 pairs (the camera in ten), medians of {rounds} interleaved rounds (selinv: the tile solves; blocks: "
        "right-hand sides and blocks)")
    mk = report(out, "covariance_pairs(), known", tk)
    mf = report(out, "..._pairs_lens(), free", tf)
    out(f"  the lens costs {mf - mk:+.3f} ms, {mf / mk:.3f} of the known-lens call")
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
