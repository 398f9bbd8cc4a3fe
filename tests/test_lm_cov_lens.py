"""CPU tests of tests/lm_cov_lens_ref.py, the numpy reference of the covariance with the lens
estimated, and the inputs tests/test_gpu_lm_cov_lens.py shares with it.

  * caps on the reference alone, on every input the GPU test uses, at the reference's own solve
    from l = (0, 0) with tag 0 constant: e_ref <= 1e-9 (the project's cap), and the smallest
    squared pivot of the reduced system >= 1e-7 in either elimination order -- seven orders above
    the device's 1e-14 threshold, so no input sits near the rank decision.
  * held lens: with the l columns dropped the helper is lm_cov_ref.covariance over
    distortion_ref.RadialOracle, exactly.
  * the covariance is the spread of the estimates: 256 noisy copies of one graph solved from the
    truth with the lens free; bounds at 4 standard errors, as tests/test_lm_cov.py.
"""
import functools

import numpy as np
import pytest

import distortion_free_ref as fref
import distortion_ref as dref
import lm_cov_lens_ref as lens_ref
import lm_cov_ref
import tag_size_ref as tref
from ar_slam_amd import synth
from loss_ref import CAUCHY
from tag_size_ref import arrays

E_REF_CAP = 1e-9       # the project's cap on the reference's own error (tests/test_lm_cov.py)
MIN_PIVOT_CAP = 1e-7   # either elimination order; the device's threshold is 1e-14


@functools.lru_cache(maxsize=None)
def graph(name):
    """The inputs: g6, g20, gk11 (distortion_ref.trace_graphs under MILD; gk11 has captures of 11
    observations of 11 distinct tags: more than kSchurMfmaBlocks tags, and chunked), the README's
    scene, and g22: 21 free tags, so the camera's three rows straddle a tile boundary."""
    if name == "scene":
        return dref.scene()
    if name == "g22":
        return synth.make_graph(22, 11, 2, seed=5, k=6, distortion=dref.MILD)
    return dref.trace_graphs(dref.MILD)[name][0]


def tag0_const(g):
    tc = np.zeros(g.n_tag, np.uint8)
    tc[0] = 1
    return tc


def losses(g, with_loss):
    """(kinds, a) per observation: Cauchy(3) on every one, or none."""
    if not with_loss:
        return 0, 0.0
    return np.full(g.n_obs, CAUCHY, np.uint8), np.full(g.n_obs, 3.0)


@functools.lru_cache(maxsize=None)
def reference_solve(oracle, name, with_loss):
    """The dense LM's solve of the input from l = (0, 0), tag 0 constant: (camera, cap, tag, summary)."""
    g = graph(name)
    kinds, a = losses(g, with_loss)
    return tref.solve(fref.FreeRadialOracle(oracle), fref.zero_lens(arrays(g)), None, False, None, tag0_const(g),
                      kinds, a)


CASES = [("g6", False), ("g20", False), ("gk11", False), ("scene", False), ("g20", True), ("g22", False)]


@pytest.mark.parametrize("name, with_loss", CASES, ids=[f"{n}{'-cauchy' if l else ''}" for n, l in CASES])
def test_reference_error_caps(oracle, name, with_loss):
    g = graph(name)
    kinds, a = losses(g, with_loss)
    cam, cap, tag, s = reference_solve(oracle, name, with_loss)
    assert s["termination"] == "CONVERGENCE"
    start = fref.zero_lens(arrays(g))
    ref = lens_ref.covariance(fref.FreeRadialOracle(oracle), (cam, cap, tag) + start[3:], False, None, tag0_const(g),
                              kinds, a, scale_arrays=start)
    print(f"{name} cauchy={with_loss}: e_ref {ref.e_ref:.2e}; smallest pivot captures first {ref.min_pivot:.2e}, "
          f"tags first {ref.min_pivot_tags:.2e}; {len(ref.cols)} free parameters")
    assert ref.e_ref <= E_REF_CAP
    assert ref.min_pivot >= MIN_PIVOT_CAP and ref.min_pivot_tags >= MIN_PIVOT_CAP
    assert ref.n_cam == 3 and list(ref.cols[:3]) == [0, 1, 2] and ref.cam_status == lens_ref.OK
    assert np.array_equal(ref.cam, ref.cam.T) and np.all(np.linalg.eigvalsh(ref.cam) > 0)
    assert ref.var_f == ref.cam[0, 0]
    assert ref.tag_status[0] == lens_ref.UNAVAILABLE and np.all(ref.tag[0] == -1.0)
    # the lens costs certainty: every marginal is at least the held lens' (a Schur complement of a larger H)
    held = lens_ref.covariance(fref.FreeRadialOracle(oracle), (cam, cap, tag) + start[3:], False, None, tag0_const(g),
                               kinds, a, scale_arrays=start, lens=False)
    assert ref.var_f > held.var_f
    ok = ref.tag_status == lens_ref.OK
    assert np.all(np.einsum("bii->bi", ref.tag[ok]) >= np.einsum("bii->bi", held.tag[ok]) * (1 - 1e-9))


def test_gk11_and_g22_are_the_shapes_they_are_used_for():
    g = graph("gk11")
    per_cap = [len(np.unique(g.obs_tag[g.obs_cap == c])) for c in range(g.n_cap)]
    assert np.bincount(g.obs_cap).max() >= 11 and max(per_cap) > 10
    g = graph("g22")
    assert g.n_tag == 22 and np.all(np.bincount(g.obs_tag, minlength=22) > 0)


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "cauchy"])
def test_held_lens_is_the_existing_reference_exactly(oracle, with_loss):
    g = graph("g20")
    kinds, a = losses(g, with_loss)
    A = arrays(g)
    tc = tag0_const(g)
    rows = (-np.ones(g.n_cap, np.int64), np.where(tc == 0, 6 * np.arange(g.n_tag)[::-1], -1), 6 * g.n_tag)
    want = lm_cov_ref.covariance(dref.RadialOracle(oracle), A, False, None, tc, kinds, a, rows=rows)
    got = lens_ref.covariance(fref.FreeRadialOracle(oracle), A, False, None, tc, kinds, a, rows=rows, lens=False)
    assert np.array_equal(got.cols, want.cols) and np.array_equal(got.C, want.C)
    assert np.array_equal(got.cap, want.cap) and np.array_equal(got.tag, want.tag)
    assert np.array_equal(got.cap_status, want.cap_status) and np.array_equal(got.tag_status, want.tag_status)
    assert got.var_f == want.var_f and got.e_ref == want.e_ref
    assert got.min_pivot == want.min_pivot and got.min_pivot_rows == want.min_pivot_rows
    assert got.cam[0, 0] == want.var_f and np.all(got.cam.ravel()[1:] == 0.0) and got.n_cam == 1
    # a constant camera: no camera block
    const = lens_ref.covariance(fref.FreeRadialOracle(oracle), A, True, None, tc, kinds, a)
    assert const.cam_status == lens_ref.UNAVAILABLE and np.all(const.cam == -1.0) and const.n_cam == 0
    assert const.pair((lens_ref.CAMERA, 0), (lens_ref.TAG, 1)) is None


def test_pair_layout():
    ref = lens_ref.LensCovRef()
    ref.nc, ref.n_cam = 1, 3
    ref.cols = np.concatenate([[0, 1, 2], 3 + np.arange(6), 15 + np.arange(6)])   # capture 0, tag 1 (tag 0 constant)
    ref.C = np.arange(15.0 * 15.0).reshape(15, 15)
    cam, cap, tag = (lens_ref.CAMERA, 0), (lens_ref.CAPTURE, 0), (lens_ref.TAG, 1)
    p = ref.pair(cam, tag)
    assert np.array_equal(p[:3], ref.C[:3, 9:15]) and np.all(p[3:] == 0.0)
    p = ref.pair(cap, cam)
    assert np.array_equal(p[:, :3], ref.C[3:9, :3]) and np.all(p[:, 3:] == 0.0)
    p = ref.pair(cam, cam)
    assert np.array_equal(p[:3, :3], ref.C[:3, :3]) and p[3:].sum() == 0.0 and p[:, 3:].sum() == 0.0
    assert ref.pair(cap, (lens_ref.TAG, 0)) is None


STAT_N = 256
STAT_SIGMA = 0.1


def test_covariance_is_the_spread_of_the_estimates(oracle):
    """256 noisy copies of one graph (detections through the MILD lens, no other noise), each
    solved from the truth with the lens free, tag 0 the anchor.  With d = estimate - truth, to
    first order the mean over the copies of d'(sigma^2 C)^-1 d is the block's size: 3 for the
    camera's [f, l1, l2] (a chi-square of 3 degrees of freedom has variance 6: standard error
    sqrt(6 / 256) = 0.153), 1 for each camera parameter (sqrt(2 / 256) = 0.088), 6 for each of the
    39 free pose blocks (sqrt(12 / 256) = 0.217).  Bounds at 4 standard errors.  C of a held lens
    is too small for the camera by far more than that."""
    g = synth.make_graph(20, 5, 4, seed=5, k=6, noise_px=0, distortion=dref.MILD)
    R = fref.FreeRadialOracle(oracle)
    tc = tag0_const(g)
    truth = (g.camera_true, g.cap_true, g.tag_true, g.obs_cap, g.obs_tag, g.corners)
    assert np.array_equal(g.camera_true[1:], dref.MILD)
    ref = lens_ref.covariance(R, truth, False, None, tc)
    s2 = STAT_SIGMA ** 2
    inv_cam = np.linalg.inv(s2 * ref.cam)
    inv_c = np.array([np.linalg.inv(s2 * ref.cap[c]) for c in range(g.n_cap)])
    inv_t = np.array([np.linalg.inv(s2 * ref.tag[t]) if not tc[t] else np.zeros((6, 6)) for t in range(g.n_tag)])
    rng = np.random.default_rng(17)
    acc_cam, acc_each = 0.0, np.zeros(3)
    acc_c, acc_t = np.zeros(g.n_cap), np.zeros(g.n_tag)
    for _ in range(STAT_N):
        corners = g.corners + rng.normal(0.0, STAT_SIGMA, g.corners.shape)
        cam, cap, tag, s = tref.solve(R, truth[:5] + (corners,), None, False, None, tc, function_tolerance=1e-14,
                                      parameter_tolerance=1e-12, max_num_iterations=200)
        assert s["termination"] == "CONVERGENCE"
        d = cam - g.camera_true
        acc_cam += d @ inv_cam @ d
        acc_each += d * d / (s2 * np.diag(ref.cam))
        dc, dt = cap - g.cap_true, tag - g.tag_true
        acc_c += np.einsum("ci,cij,cj->c", dc, inv_c, dc)
        acc_t += np.einsum("ci,cij,cj->c", dt, inv_t, dt)
    means = np.concatenate([acc_c, acc_t[~tc.astype(bool)]]) / STAT_N
    each = acc_each / STAT_N
    print(f"camera block mean {acc_cam / STAT_N:.3f} (3 +- {4 * np.sqrt(6.0 / STAT_N):.2f}); f, l1, l2 "
          f"{each[0]:.3f} / {each[1]:.3f} / {each[2]:.3f} (1 +- {4 * np.sqrt(2.0 / STAT_N):.2f}); "
          f"pose blocks {means.min():.3f} .. {means.max():.3f} over {len(means)} (6 +- {4 * np.sqrt(12.0 / STAT_N):.2f})")
    assert len(means) == 39
    assert abs(acc_cam / STAT_N - 3.0) <= 4.0 * np.sqrt(6.0 / STAT_N)
    assert np.all(np.abs(each - 1.0) <= 4.0 * np.sqrt(2.0 / STAT_N)), each
    assert np.all(np.abs(means - 6.0) <= 4.0 * np.sqrt(12.0 / STAT_N)), means
