"""Records tests/golden/schur_k1to11.npz with the library ARSLAM_LIB names (the build whose results
tests/test_gpu_schur_store.py then requires bit for bit): a graph whose captures see 1..11 distinct
tags in turn, solved with captures eliminated -- all blocks free, and with one tag and the camera
held constant.
usage: ARSLAM_LIB=... python tools/make_schur_golden.py out.npz"""
import sys

import numpy as np

sys.path.insert(0, ".")
from ar_slam_amd import lm, synth  # noqa: E402


def graph():
    return synth.make_graph(44, 8, 6, 33, k=tuple(range(1, 12)), depth=(1.2, 2.0))


def const_blocks(g):
    """(camera_const, tag_const) of the second case: the first observation's tag and the camera."""
    tc = np.zeros(g.n_tag, np.uint8)
    tc[g.obs_tag[0]] = 1
    return True, tc


def solve(g, const):
    kw = {}
    if const:
        kw["camera_const"], kw["tag_const"] = const_blocks(g)
    return lm.solve_soa(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, elimination=lm.ELIM_CAPTURES, **kw)


if __name__ == "__main__":
    g = graph()
    out = {}
    for tag, const in (("free", False), ("const", True)):
        cam, cap, tg, s = solve(g, const)
        out[f"{tag}_cost"] = np.array([i["cost"] for i in s["iterations"]], np.float64)
        out[f"{tag}_camera"], out[f"{tag}_cap"], out[f"{tag}_tag"] = cam, cap, tg
        print(tag, s["termination"], len(s["iterations"]), s["num_linear_solves"], repr(s["final_cost"]))
    np.savez_compressed(sys.argv[1], **out)
    print(lm.library_info())
