"""What the mapper's marginal covariances cost on cfg3 (debug / profiles/lm_cov).

One process, one resident handle on cfg3 with tag 0 held constant (the anchor): a warm-up solve
and covariance, then ROUNDS rounds of solve() + covariance().  Prints the four device times of a
covariance call (HIP events: linearization, reduced system + factorization, selected inverse,
marginal blocks), one LM iteration's device time of the same problem (the solve's phase timers
over its linear solves), their ratio, the tile products of the selected inverse against the
factorization's, and the fp64 MFMA rate the selected inverse's time implies.  Then, on the same
handle, covariance_pairs() for one pair and for 100 pairs over distinct tags (profiles/lm_cov_pairs):
its device times, its tile products against the selected inverse's, and the host wall time of a call.

usage: python tools/lm_cov_cost.py [rounds] [config]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ar_slam_amd import lm, synth  # noqa: E402

PHASES = ["t_linearize_ms", "t_factor_ms", "t_selinv_ms", "t_blocks_ms"]


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    name = sys.argv[2] if len(sys.argv) > 2 else "cfg3"
    g = synth.config_graph(name)
    tag_const = np.zeros(g.n_tag, np.uint8)
    tag_const[0] = 1
    rp = lm.ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, tag_const=tag_const,
                            phase_timing=1)
    t = {p: [] for p in PHASES}
    it_ms = []
    for r in range(1 + rounds):
        s = rp.solve()
        out = rp.covariance()
        if r == 0:
            continue
        for p in PHASES:
            t[p].append(out["info"][p])
        dev = sum(s[k] for k in ("t_linearize_ms", "t_schur_ms", "t_cholesky_ms", "t_solve_ms", "t_backsub_ms",
                                 "t_cost_ms"))
        it_ms.append(dev / max(s["num_linear_solves"], 1))
    info = out["info"]
    ok_c = out["cap_status"] == lm.COV_OK
    ok_t = out["tag_status"] == lm.COV_OK
    print(f"{name}: {g.n_cap} captures, {g.n_tag} tags, {g.n_obs} observations, tag 0 constant; elimination "
          f"{s['elimination_used']}, {info['n_reduced']} reduced rows, {info['n_factor_tiles']} factor tiles; "
          f"status {info['status']}, min_pivot {info['min_pivot']:.3e}; {ok_c.sum()} capture and {ok_t.sum()} tag blocks")
    print(f"medians of {rounds} rounds (min - max), device ms by HIP events")
    total = np.zeros(rounds)
    for p in PHASES:
        v = np.array(t[p])
        total += v
        print(f"  {p[2:-3]:10s} {np.median(v):9.3f} ({v.min():.3f} - {v.max():.3f})")
    it = np.array(it_ms)
    print(f"  {'total':10s} {np.median(total):9.3f} ({total.min():.3f} - {total.max():.3f})")
    print(f"  one LM iteration of the same problem {np.median(it):.3f} ({it.min():.3f} - {it.max():.3f}): "
          f"a covariance call = {np.median(total) / np.median(it):.2f} LM iterations")
    sel, fac = info["n_selinv_products"], info["n_factor_products"]
    tf = 2.0 * 64 ** 3 * sel / (1e-3 * np.median(t["t_selinv_ms"])) / 1e12 if sel else 0.0
    print(f"  tile products (64x64x64): selected inverse {sel}, factorization {fac}, ratio {sel / max(fac, 1):.2f}; "
          f"the selected inverse's time implies {tf:.2f} TFLOP/s fp64")
    pos = np.sqrt(np.einsum("bii->b", out["tag"][ok_t][:, :3, :3]))
    print(f"  1-sigma tag position at 0.5 px: median {500 * np.median(pos):.3f} mm, largest {500 * pos.max():.3f} mm; "
          f"sigma_f {0.5 * np.sqrt(out['var_f']):.4f} px")
    pairs_cost(rp, rounds, np.median(total), sel, np.nonzero(ok_t)[0])


def pairs_cost(rp, rounds, cov_total_ms, selinv_products, tags):
    """covariance_pairs() on the same handle, in the same process: one pair, and 100 pairs over 200
    distinct tags (100 solved blocks: ten panels, three batches)."""
    lists = {"1 pair": [((lm.BLOCK_TAG, int(tags[0])), (lm.BLOCK_TAG, int(tags[len(tags) // 2])))],
             "100 pairs": [((lm.BLOCK_TAG, int(tags[2 * k])), (lm.BLOCK_TAG, int(tags[2 * k + 1]))) for k in range(100)]}
    print(f"covariance_pairs on the same handle, medians of {rounds} rounds (min - max), device ms by HIP events "
          "(selinv: the tile solves; blocks: right-hand sides and blocks)")
    for label, pairs in lists.items():
        t = {p: [] for p in PHASES}
        wall = []
        for r in range(1 + rounds):
            rp.solve()
            t0 = time.perf_counter()
            cov, st, info = rp.covariance_pairs(pairs)
            t1 = time.perf_counter()
            assert np.all(st == lm.COV_OK)
            if r == 0:
                continue
            wall.append(1e3 * (t1 - t0))
            for p in PHASES:
                t[p].append(info[p])
        total = np.zeros(rounds)
        line = []
        for p in PHASES:
            v = np.array(t[p])
            total += v
            line.append(f"{p[2:-3]} {np.median(v):.3f} ({v.min():.3f} - {v.max():.3f})")
        prod = info["n_selinv_products"]
        tf = 2.0 * 64 ** 3 * prod / (1e-3 * np.median(t["t_selinv_ms"])) / 1e12
        print(f"  {label:9s} " + "; ".join(line))
        print(f"  {'':9s} total {np.median(total):.3f} ({total.min():.3f} - {total.max():.3f}) = "
              f"{np.median(total) / cov_total_ms:.2f} of a covariance() call; host wall {np.median(wall):.3f} ms; "
              f"tile products {prod} = {prod / max(selinv_products, 1):.2f} of the selected inverse's {selinv_products}; "
              f"the solves' time implies {tf:.2f} TFLOP/s fp64")


if __name__ == "__main__":
    main()
