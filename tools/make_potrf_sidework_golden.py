"""Records tests/golden/potrf_sidework_parent.npz with the library ARSLAM_LIB names (the build whose
results tests/test_gpu_potrf_sidework.py then requires bit for bit): the `medium` graph (200 captures)
solved by the persistent executor -- the cost of every LM iteration, the final camera, capture poses
and tag poses, and how the solve ended.  The file holds those values only.
usage: ARSLAM_LIB=... python tools/make_potrf_sidework_golden.py out.npz"""
import sys

import numpy as np

sys.path.insert(0, ".")

GRAPH = "medium"


def solve(lm, **kw):
    """The persistent executor's solve of GRAPH: dict of cost trace, final parameters, termination."""
    from ar_slam_amd import synth
    g = synth.config_graph(GRAPH)
    rp = lm.ResidentProblem(camera=g.camera, cap=g.cap, tag=g.tag, obs_cap=g.obs_cap, obs_tag=g.obs_tag,
                            corners=g.corners, factor_executor=1, **kw)
    try:
        s = rp.solve()
        return dict(cost=np.array([it["cost"] for it in s["iterations"]], np.float64), camera=rp.camera.copy(),
                    cap=rp.cap.copy(), tag=rp.tag.copy(), termination=np.array(str(s["termination"])),
                    rule=np.array(str(s["rule"])), num_linear_solves=np.array(s["num_linear_solves"], np.int64))
    finally:
        rp.close()


if __name__ == "__main__":
    from ar_slam_amd import lm
    out = solve(lm)
    again = solve(lm)
    for k in out:   # (a recording that the recording build itself does not repeat would pin nothing)
        assert out[k].tobytes() == again[k].tobytes(), k
    np.savez_compressed(sys.argv[1], graph=np.array(GRAPH), **out)
    print("cost trace", out["cost"], "termination", out["termination"], out["rule"])
    print(lm.library_info())
