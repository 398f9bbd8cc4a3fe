"""GPU tests of the SLAM mirror's mapper covariance (arslam_slam_covariance and its getters,
arslam_slam_covariance_pair; include/arslam_slam.h): `small` through SlamSolver.solve() at the
mirror's default elimination (Ceres' mixed e-block set), then the covariance in the gauge of aruco 0.

The reference problem is built from arslam_slam_block at the poses the mirror returned, with that
aruco constant (tests/lm_cov_ref.py, tests/lm_cov_pairs_ref.py), and held to the bound of
tests/test_gpu_lm_cov.py: |C_dev - C_ref|_ij <= tol sqrt(C_ii C_jj), tol = max(16 e_ref, 1e-10).
The Jacobi scale of the reference is that of the returned point (the handle's is that of its last
solve's start, which the mirror does not expose; C does not depend on the scale beyond rounding).
"""
import ctypes as C

import numpy as np
import pytest

import lm_cov_pairs_ref as pairs_ref
import lm_cov_ref as cov_ref
from ar_slam_amd import synth
from test_gpu_slam import _detections
from test_lm_cov import E_REF_CAP

pytestmark = pytest.mark.gpu

CAMERA, CAPTURE, TAG = 0, 1, 2
STATE, INVALID_ARG = -7, -1


def _solved(lm, g, caps=None):
    s = lm.SlamSolver()
    s.set_camera(g.camera)
    for uid, ids, corners in _detections(g, caps):
        s.add_detections(uid, ids, corners)
    s.solve()
    return s


def _problem_arrays(s):
    """The mapper problem from arslam_slam_block: the added blocks, at the mirror's poses."""
    blocks = [s.block(b) for b in range(s.num_blocks)]
    added = [(c, a, rect) for c, a, rect, ok in blocks if ok]
    obs_cap = np.array([c for c, _, _ in added], np.int32)
    obs_tag = np.array([a for _, a, _ in added], np.int32)
    corners = np.array([rect for _, _, rect in added])
    return (s.camera()[0], s.capture_poses(), s.aruco_poses(), obs_cap, obs_tag, corners)


def test_covariance_in_the_gauge_of_aruco_0(lm, oracle):
    g = synth.config_graph("small")
    s = _solved(lm, g)
    used = {s.solve_summary(i)["elimination_used"] for i in range(s.num_solves)}
    assert s.last_summary()["elimination_used"] == lm.ELIM_MIXED, used
    arrays = _problem_arrays(s)
    assert len(arrays[3]) == g.n_obs
    tc = np.zeros(s.num_arucos, np.uint8)
    tc[0] = 1
    ref = cov_ref.covariance(oracle, arrays, False, np.zeros(s.num_captures, np.uint8), tc)
    assert ref.e_ref <= E_REF_CAP
    tol = max(16.0 * ref.e_ref, 1e-10)
    out = s.covariance(0)
    assert out["info"]["status"] == lm.COV_OK and out["info"]["min_pivot"] > 1e-14
    assert np.array_equal(out["cap_status"], ref.cap_status) and np.array_equal(out["aruco_status"], ref.tag_status)
    assert out["aruco_status"][0] == lm.COV_UNAVAILABLE and np.all(out["aruco"][0] == -1.0)
    worst = 0.0
    for dev, want, st in ((out["cap"], ref.cap, ref.cap_status), (out["aruco"], ref.tag, ref.tag_status)):
        ok = st == lm.COV_OK
        assert np.all(dev[~ok] == -1.0)
        assert np.array_equal(dev[ok], np.transpose(dev[ok], (0, 2, 1)))
        d = np.sqrt(np.einsum("bii->bi", want[ok]))
        worst = max(worst, float(np.max(np.abs(dev[ok] - want[ok]) / (d[:, :, None] * d[:, None, :]))))
    cam = out["cam"]
    assert out["cam_status"] == lm.COV_OK and np.all(cam.ravel()[1:] == 0.0)
    worst = max(worst, abs(cam[0, 0] - ref.var_f) / ref.var_f)
    # a cross block: a capture against an aruco it sees, and the camera against an aruco
    c, a = int(arrays[3][-1]), int(arrays[4][-1])
    pairs = [((CAPTURE, c), (TAG, a)), ((CAMERA, 0), (TAG, a))]
    pref = pairs_ref.covariance_pairs(oracle, arrays, pairs, False, np.zeros(s.num_captures, np.uint8), tc)
    worst_p = 0.0
    for p, (ba, bb) in enumerate(pairs):
        cov, st = s.covariance_pair(0, ba, bb)
        assert st == pref.status[p] == lm.COV_OK
        worst_p = max(worst_p, float(np.max(np.abs(cov - pref.cov[p]) / pref.scale[p])))
        back, _ = s.covariance_pair(0, bb, ba)
        assert np.array_equal(back, cov.T)
    print(f"mirror, small, anchor aruco 0: blocks {worst:.2e}, pairs {worst_p:.2e} (tol {tol:.2e}, e_ref {ref.e_ref:.2e}, "
          f"e_ref_pairs {pref.e_ref_pairs:.2e}); min_pivot {out['info']['min_pivot']:.3e}, {out['info']['n_reduced']} reduced rows")
    assert worst <= tol and worst_p <= max(tol, 16.0 * pref.e_ref_pairs)
    cov, st = s.covariance_pair(0, (TAG, 0), (TAG, 1))
    assert st == lm.COV_UNAVAILABLE and np.all(cov == -1.0)
    # the kept result is served again, bit for bit; another anchor is another gauge
    again = s.covariance(0)
    assert np.array_equal(again["cap"], out["cap"]) and np.array_equal(again["aruco"], out["aruco"])
    other = s.covariance(1)
    assert other["aruco_status"][1] == lm.COV_UNAVAILABLE and other["aruco_status"][0] == lm.COV_OK
    assert abs(other["cam"][0, 0] - cam[0, 0]) <= 2 * tol * cam[0, 0]      # var(f) does not depend on the gauge


def test_rules(lm):
    g = synth.config_graph("small")
    first_loc = g.n_cap - 3
    s = lm.SlamSolver()
    s.set_camera(g.camera)
    with pytest.raises(lm.LMError) as e:
        s.covariance(0)
    assert e.value.code in (STATE, INVALID_ARG)          # nothing added yet
    for uid, ids, corners in _detections(g, range(first_loc)):
        s.add_detections(uid, ids, corners)
    s.solve()
    for uid, ids, corners in _detections(g, range(first_loc, g.n_cap)):
        s.add_detections(uid, ids, corners)
    s.localize_many(first_loc)
    out = s.covariance(0)
    assert out["info"]["status"] == lm.COV_OK
    # the captures localize_many localized are not in the mapper problem
    assert np.all(out["cap_status"][first_loc:] == lm.COV_UNAVAILABLE) and np.all(out["cap"][first_loc:] == -1.0)
    assert np.all(out["cap_status"][:first_loc] == lm.COV_OK)
    cov, st = s.covariance_pair(0, (CAPTURE, g.n_cap - 1), (TAG, 1))
    assert st == lm.COV_UNAVAILABLE and np.all(cov == -1.0)
    # the anchor: an aruco with residual blocks in the problem
    for bad in (-1, s.num_arucos, 10 ** 6):
        with pytest.raises(lm.LMError) as e:
            s.covariance(bad)
        assert e.value.code == INVALID_ARG
        with pytest.raises(lm.LMError) as e:
            s.covariance_pair(bad, (TAG, 1), (TAG, 2))
        assert e.value.code == INVALID_ARG
    for a, b in (((7, 0), (TAG, 1)), ((TAG, s.num_arucos), (TAG, 1)), ((CAMERA, 1), (TAG, 1))):
        with pytest.raises(lm.LMError) as e:
            s.covariance_pair(0, a, b)
        assert e.value.code == INVALID_ARG
    # a failed call keeps nothing; after a good one, a change of the problem drops the kept result
    cov6, cov9, st = np.zeros((6, 6)), np.zeros((3, 3)), C.c_int(0)
    p6 = cov6.ctypes.data_as(C.POINTER(C.c_double))
    assert lm.lib().arslam_slam_aruco_covariance(s._h, 1, p6, C.byref(st)) == STATE
    s.covariance(0)
    assert lm.lib().arslam_slam_aruco_covariance(s._h, 1, p6, C.byref(st)) == 0 and st.value == lm.COV_OK
    assert lm.lib().arslam_slam_aruco_covariance(s._h, s.num_arucos, p6, C.byref(st)) == INVALID_ARG
    s.add_detections("one_more", ["tag_1"], g.corners[:1])
    assert lm.lib().arslam_slam_aruco_covariance(s._h, 1, p6, C.byref(st)) == STATE
    assert lm.lib().arslam_slam_capture_covariance(s._h, 0, p6, C.byref(st)) == STATE
    assert lm.lib().arslam_slam_camera_covariance(s._h, cov9.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)) == STATE
