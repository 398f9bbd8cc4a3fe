"""Per-query pose covariance of the batched localizer without a GPU: the new entry points are
exported and answer STATE before any device call, the numpy reference (tests/localize_cov_ref.py)
is the plain inverse of J'J (of the rows scaled by sqrt(rho') under losses), and the covariance
means what it says: over many noisy copies of one query the pose error d satisfies
mean d' (sigma^2 C)^-1 d = 6.
"""
import ctypes as C
import time

import numpy as np
import pytest

import localize_cov_ref as cov_ref
import localize_ref
import loss_ref
from ar_slam_amd import synth

STATE = -7
NEW_SYMBOLS = ["arslam_localizer_covariance", "arslam_localizer_covariance_timed", "arslam_localize_many_cov",
               "arslam_slam_localize_covariance"]
SIGMA = 0.5          # px, the noise of the statistical check
STAT_SEED = 20
STAT_N = 6144        # copies in the CPU statistical check (about 27 s through localize_ref)


@pytest.fixture(scope="module")
def L():
    from ar_slam_amd import build, lm
    build.build()
    lm.lib()
    return lm


def test_new_symbols_are_exported(L):
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTS
        assert hasattr(L.lib(), name), name


def test_covariance_needs_a_solve(L):
    """Nothing loaded: STATE, also on a host without a GPU (checked before any device call)."""
    h = C.c_void_p()
    assert L.lib().arslam_localizer_create(C.byref(h), C.byref(L.make_options())) == 0
    try:
        cov, st, mp = np.zeros(36), np.zeros(1, np.int32), np.zeros(1)
        assert L.lib().arslam_localizer_covariance(h, None, None, None) == STATE
        assert L.lib().arslam_localizer_covariance(h, cov.ctypes.data_as(L._dp), st.ctypes.data_as(L._ip),
                                                   mp.ctypes.data_as(L._dp)) == STATE
        assert L.lib().arslam_localizer_covariance_timed(h, None, None, None, None) == STATE
        assert (cov == 0.0).all()
    finally:
        L.lib().arslam_localizer_destroy(h)


def test_slam_mirror_covariance_needs_a_localize(L):
    s = L.SlamSolver()
    try:
        cov = np.zeros(36)
        assert L.lib().arslam_slam_localize_covariance(s._h, 0, cov.ctypes.data_as(L._dp), None) == STATE
        assert L.lib().arslam_slam_localize_covariance(s._h, -1, None, None) == -1
    finally:
        s.close()


def _rel(C_, R):
    d = np.sqrt(np.einsum("qi,qj->qij", np.einsum("qii->qi", R), np.einsum("qii->qi", R)))
    return np.abs(C_ - R) / d


def test_reference_is_the_plain_inverse(oracle):
    """Clean 64-query batch at the true poses: the helper equals inv(J'J) of the plain Jacobians."""
    b = synth.make_localize_batch(n_query=64)
    cov, st, mp = cov_ref.covariance(oracle, b, b.pose_true)
    assert (st == cov_ref.OK).all() and (mp > 0).all() and (mp <= 1.0).all()
    ref = np.zeros_like(cov)
    for q, a, e, qr in localize_ref._queries(oracle, b, None, None):
        _, J = qr.plain(b.pose_true[q])
        J = J.reshape(-1, 6)
        ref[q] = np.linalg.inv(J.T @ J)
    err = _rel(cov, ref).max()
    print("relative to sqrt(C_ii C_jj):", err, "min_pivot", mp.min(), mp.max())
    assert err <= 1e-10
    np.testing.assert_array_equal(cov, cov.transpose(0, 2, 1))


def test_reference_under_per_observation_losses(oracle):
    """Rows scaled by sqrt(rho'(s)) per observation, each observation its own kind and scale, on
    queries with one observation shifted by 40 px."""
    b, _ = localize_ref.shifted_batch(synth.make_localize_batch(n_query=32), seed=11, px=40.0)
    o = np.arange(b.n_obs)
    kinds, scales = (o % 4).astype(np.uint8), 2.0 + (o % 3)
    cov, st, mp = cov_ref.covariance(oracle, b, b.pose_true, kinds, scales)
    assert (st == cov_ref.OK).all()
    ref = np.zeros_like(cov)
    differs = 0.0
    for q, a, e, qr in localize_ref._queries(oracle, b, None, None):
        r, J = qr.plain(b.pose_true[q])
        rows = []
        for j in range(e - a):
            _, rho1 = loss_ref.rho(int(kinds[a + j]), float(scales[a + j]), float(r[j] @ r[j]))
            rows.append(np.sqrt(float(rho1)) * J[j])
        Jt = np.concatenate(rows)
        ref[q] = np.linalg.inv(Jt.T @ Jt)
        Jp = J.reshape(-1, 6)
        differs = max(differs, np.abs(ref[q] / np.linalg.inv(Jp.T @ Jp) - 1.0).max())
    err = _rel(cov, ref).max()
    print("relative to sqrt(C_ii C_jj):", err, "; against the covariance without the losses:", differs)
    assert err <= 1e-10
    assert differs > 0.05          # the losses do change it


def test_rank_deficient_and_unavailable_in_the_reference():
    H = np.diag([1.0, 4.0, 9.0, 1.0, 1.0, 1.0])
    H[0, 1] = H[1, 0] = 2.0                       # rows 0 and 1 dependent: pivot 1 is 0
    cov, st, mp = cov_ref.invert(H)
    assert st == cov_ref.RANK_DEFICIENT and (cov == -1.0).all() and abs(mp) < 1e-15
    H = np.eye(6)
    H[3, 3] = 0.0
    assert cov_ref.invert(H)[1:] == (cov_ref.RANK_DEFICIENT, -1.0)
    H[3, 3] = np.inf
    assert cov_ref.invert(H)[1:] == (cov_ref.RANK_DEFICIENT, -1.0)
    cov, st, mp = cov_ref.invert(np.diag([1.0, 2.0, 4.0, 8.0, 16.0, 32.0]))
    assert st == cov_ref.OK and mp == 1.0
    np.testing.assert_allclose(np.diag(cov), 1.0 / np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0]), rtol=1e-15)


def stat_batch(n, q=1):
    """The statistical check's input: query q of the noise-free 4-query batch, n noisy copies."""
    base = synth.make_localize_batch(n_query=4, noise_px=0.0)
    return cov_ref.replicated_batch(base, q, n, SIGMA, STAT_SEED)


def test_covariance_predicts_the_pose_error(oracle):
    """m = mean d' (sigma^2 C_q)^-1 d over STAT_N noisy copies of one query, solved without a loss:
    each term is chi^2_6 to first order, so m = 6 with standard error sqrt(12 / N)."""
    b = stat_batch(STAT_N)
    t0 = time.time()
    ref = localize_ref.localize(oracle, b)
    assert (ref["status"] == 0).all()
    cov, st, _ = cov_ref.covariance(oracle, b, ref["pose"], status=ref["status"], rule=ref["rule"])
    assert (st == cov_ref.OK).all()
    m = cov_ref.chi2_terms(cov, ref["pose"], b.pose_true, SIGMA).mean()
    se = np.sqrt(12.0 / STAT_N)
    sd = SIGMA * np.sqrt(np.einsum("qii->qi", cov)).mean(0)
    print(f"N = {STAT_N}: m = {m:.3f}, standard error {se:.3f}, {time.time() - t0:.1f} s; "
          f"1 sigma at {SIGMA} px: t {sd[:3] * 1e3} mm, w {sd[3:] * 1e3} mrad")
    assert abs(m - 6.0) <= 3.0 * se
