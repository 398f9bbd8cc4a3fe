"""GPU tests of the batched localizer's per-query pose covariance
(arslam_localizer_covariance, include/arslam_localize.h) against the numpy restatement of its
definition in tests/localize_cov_ref.py.

In every test the reference is evaluated at the poses the device returned, so the two differ by
rounding alone.  Tolerances (fp64):
  * |C_dev - C_ref|_ij <= 1e-9 sqrt(C_ref,ii C_ref,jj).  The relative error of the inverse is
    about kappa(Hs) * (error of the sums) with kappa(Hs) <= 6 / min_pivot; at min_pivot >= 1e-4
    and 64 * 8 rows, whose rounding errors add up like sqrt(rows) eps = 2.5e-15, that is
    1.5e-10 (3.4e-9 if all 512 added up one way), so every parity input is asserted to have a
    reference min_pivot >= 1e-4;
  * min_pivot 1e-12 absolute;
  * statuses equal.
No input sits near the rank threshold 1e-14: every reference pivot is asserted > 1e-10, except
the rank-deficient query's, which is asserted < 1e-15.
"""
import numpy as np
import pytest

import localize_cov_ref as cov_ref
import localize_ref
import loss_ref
from ar_slam_amd import synth
from test_localize_cov import SIGMA, STAT_N, stat_batch

pytestmark = pytest.mark.gpu

RESULT_FIELDS = ["status", "rule", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "init_obs",
                 "initial_cost", "final_cost"]
# single observations of b40 (query, block) whose one-tag pose has a min_pivot >= 2e-4 (most single
# tags give 1e-6 .. 1e-4: one tag seen from afar determines the pose poorly)
K1_SOURCES = [(1, 7), (1, 5), (1, 6), (10, 7)]
INSTANCES = {"k_localize_cov<2,32>": (1, 8, 5, 7), "k_localize_cov<2,64>": (1, 9, 16, 8, 12),
             "k_localize_cov<8,64>": (1, 17, 64, 8, 16, 33)}


@pytest.fixture(scope="module")
def b40():
    return synth.make_localize_batch(n_query=40, k=8)


@pytest.fixture(scope="module")
def clean96():
    return synth.make_localize_batch(n_query=96)


@pytest.fixture(scope="module")
def shifted96(clean96):
    return localize_ref.shifted_batch(clean96, seed=11, px=40.0)[0]


def _prefix(b, n):
    e = int(b.q_start[n])
    return synth.LocalizeBatch(b.camera, b.tag, b.q_start[:n + 1].copy(), b.obs_tag[:e].copy(), b.corners[:e].copy(),
                               b.pose_true[:n].copy(), b.tag_in_map.copy())


def ragged(b40, sizes, n=33, seed=2):
    """n queries of the given sizes in turn, built as test_gpu_localize_loss._ragged builds its
    batch (one real capture's observations, repeated past 8; per-observation losses kind o % 4,
    scale 2 + o % 3; every non-first observation with o % 5 == 2 shifted 40 px), except that a
    query of one observation takes one of K1_SOURCES."""
    rng = np.random.default_rng(seed)
    q_start, obs_tag, corners, n1 = [0], [], [], 0
    for i in range(n):
        k = sizes[i % len(sizes)]
        src = int(rng.integers(0, b40.n_query))
        take = [b40.q_start[src] + (j % 8) for j in range(k)]
        if k == 1:
            take = [b40.q_start[K1_SOURCES[n1 % len(K1_SOURCES)][0]] + K1_SOURCES[n1 % len(K1_SOURCES)][1]]
            n1 += 1
        obs_tag.extend(b40.obs_tag[take])
        corners.extend(b40.corners[take])
        q_start.append(q_start[-1] + k)
    corners = np.array(corners).reshape(-1, 8)
    o = np.arange(corners.shape[0])
    first = np.zeros(len(o), bool)
    first[np.array(q_start[:-1])] = True
    for i in o[(o % 5 == 2) & ~first]:
        ang = rng.uniform(0, 2 * np.pi)
        corners[i] += np.tile([40.0 * np.cos(ang), 40.0 * np.sin(ang)], 4)
    rb = synth.LocalizeBatch(b40.camera, b40.tag, np.array(q_start, np.int32), np.array(obs_tag, np.int32),
                             corners, np.zeros((n, 6)), b40.tag_in_map)
    return rb, (o % 4).astype(np.uint8), 2.0 + (o % 3)


def far_tag_batch(b40):
    """Three queries for init_from_map = 0: two of b40's at their true poses and, between them (so
    it shares a two-queries-per-wave wavefront with a live one), one that sees a single tag from
    1e9 m straight ahead: finite residuals, and an equilibrated J'J whose translation and
    rotation columns are parallel to rounding.  Returns (batch, initial poses)."""
    e = int(b40.q_start[1])
    o2 = slice(int(b40.q_start[2]), int(b40.q_start[3]))
    obs_tag = np.concatenate([b40.obs_tag[:e], b40.obs_tag[:1], b40.obs_tag[o2]]).astype(np.int32)
    corners = np.concatenate([b40.corners.reshape(-1, 8)[:e], np.zeros((1, 8)), b40.corners.reshape(-1, 8)[o2]])
    far = np.array([0.0, 0.0, 1e9, 0.0, 0.0, 0.0])
    pose0 = np.stack([b40.pose_true[0], far, b40.pose_true[2]])
    b = synth.LocalizeBatch(b40.camera, b40.tag, np.array([0, e, e + 1, e + 1 + 8], np.int32), obs_tag, corners,
                            pose0.copy(), b40.tag_in_map)
    return b, pose0


def check_against_ref(oracle, batch, pose, res, cov, st, mp, kinds=None, scales=None, parity=True):
    """The device's (cov, st, mp) against the reference at the device's poses; returns the
    reference's (cov, st, mp)."""
    c_ref, s_ref, m_ref = cov_ref.covariance(oracle, batch, pose, kinds, scales, res["status"], res["rule"])
    np.testing.assert_array_equal(st, s_ref)
    ok = s_ref == cov_ref.OK
    assert ok.any()
    assert (m_ref[ok] > 1e-10).all(), m_ref[ok].min()          # nothing near the rank threshold
    if parity:
        assert (m_ref[ok] >= 1e-4).all(), m_ref[ok].min()      # the 1e-9 below rests on this
    d = np.sqrt(np.einsum("qii->qi", c_ref[ok]))
    err = (np.abs(cov[ok] - c_ref[ok]) / (d[:, :, None] * d[:, None, :])).max()
    d_mp = np.abs(mp[ok] - m_ref[ok]).max() if mp is not None else np.nan
    print(f"{ok.sum()} queries: covariance {err:.2e} relative to sqrt(C_ii C_jj), min_pivot {d_mp:.2e} absolute, "
          f"reference min_pivot >= {m_ref[ok].min():.2e}")
    assert err <= 1e-9
    if mp is not None:
        assert np.abs(mp[ok] - m_ref[ok]).max() <= 1e-12
    assert (cov[~ok] == -1.0).all()
    return c_ref, s_ref, m_ref


def assert_well_formed(cov, st, mp):
    """Exactly symmetric; all finite and a positive diagonal where the status is OK; -1 elsewhere."""
    np.testing.assert_array_equal(cov, cov.transpose(0, 2, 1))
    ok = st == cov_ref.OK
    assert np.isfinite(cov[ok]).all()
    assert (np.einsum("qii->qi", cov[ok]) > 0.0).all()
    assert ((mp[ok] > 0.0) & (mp[ok] <= 1.0)).all()
    assert (cov[~ok] == -1.0).all()


@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "per_observation_losses"])
@pytest.mark.parametrize("name", list(INSTANCES))
def test_parity_on_every_instance(lm, oracle, b40, name, with_loss):
    """33 ragged queries (the last two-queries-per-wave wavefront holds one), k = 1, both ends of
    the instance's range and, on the 8-chunk one, the ABI's limit k = 64."""
    rb, kinds, scales = ragged(b40, INSTANCES[name])
    loc = lm.Localizer(rb, obs_loss=(kinds, scales) if with_loss else None)
    pose, res, _ = loc.solve()
    assert (res["status"] == 0).all()
    cov, st, mp = loc.covariance()
    assert (st == lm.COV_OK).all()
    assert_well_formed(cov, st, mp)
    check_against_ref(oracle, rb, pose, res, cov, st, mp, *((kinds, scales) if with_loss else (None, None)))


def test_skipped_beside_live(lm, oracle, b40):
    """Skipped queries at even and odd indices (each sharing a wavefront with a live query, one
    wavefront skipped whole, one alone in the last): status 1 and -1 everywhere; the live queries
    get the bits they get in the batch without skipped ones."""
    b = _prefix(b40, 33)
    nt = b.tag.shape[0]
    skipped = np.array([4, 7, 10, 11, 32])
    # the skipped queries see copies of their tags that no mapping capture saw, so no live query
    # loses a tag (or its initial block) to the cleared flags
    obs_tag = b.obs_tag.copy()
    for q in skipped:
        obs_tag[b.q_start[q]:b.q_start[q + 1]] += nt
    mixed = synth.LocalizeBatch(b.camera, np.concatenate([b.tag, b.tag]), b.q_start, obs_tag, b.corners, b.pose_true,
                                np.concatenate([np.ones(nt, np.uint8), np.zeros(nt, np.uint8)]))
    loc = lm.Localizer(mixed)
    pose, res, _ = loc.solve()
    cov, st, mp = loc.covariance()
    sk = np.zeros(33, bool)
    sk[skipped] = True
    np.testing.assert_array_equal(res["status"] == lm.LOC_SKIPPED, sk)
    assert (st[sk] == lm.COV_UNAVAILABLE).all() and (cov[sk] == -1.0).all() and (mp[sk] == -1.0).all()
    assert (st[~sk] == lm.COV_OK).all()
    assert_well_formed(cov, st, mp)
    loc0 = lm.Localizer(b)
    pose0, _, _ = loc0.solve()
    cov0, st0, mp0 = loc0.covariance()
    np.testing.assert_array_equal(pose[~sk], pose0[~sk])
    np.testing.assert_array_equal(cov[~sk], cov0[~sk])
    np.testing.assert_array_equal(mp[~sk], mp0[~sk])
    check_against_ref(oracle, mixed, pose, res, cov, st, mp)
    # the same under a loss (the kLoss instance's half-wave exit)
    loc.set_loss(lm.LOSS_HUBER, 3.0)
    pose, res, _ = loc.solve()
    cov, st, mp = loc.covariance()
    assert (st[sk] == lm.COV_UNAVAILABLE).all() and (cov[sk] == -1.0).all() and (mp[sk] == -1.0).all()
    check_against_ref(oracle, mixed, pose, res, cov, st, mp, loss_ref.HUBER, 3.0)


def test_rank_deficient(lm, oracle, b40):
    """One tag from 1e9 m: the equilibrated Cholesky loses a pivot to rounding -> status 2, -1
    everywhere and the offending pivot; its wave partner and the third query are untouched."""
    b, pose0 = far_tag_batch(b40)
    loc = lm.Localizer(b, init_from_map=False, pose=pose0, max_num_iterations=0)
    pose, res, _ = loc.solve()
    np.testing.assert_array_equal(pose, pose0)
    assert np.isfinite(res["final_cost"]).all() and (res["status"] == 1).all()      # NO_CONVERGENCE
    cov, st, mp = loc.covariance()
    c_ref, s_ref, m_ref = cov_ref.covariance(oracle, b, pose, status=res["status"], rule=res["rule"])
    print("pivot of the far query: device", mp[1], "reference", m_ref[1], "; the others", mp[[0, 2]], m_ref[[0, 2]])
    assert s_ref[1] == cov_ref.RANK_DEFICIENT and m_ref[1] < 1e-15
    np.testing.assert_array_equal(st, [lm.COV_OK, lm.COV_RANK_DEFICIENT, lm.COV_OK])
    assert (cov[1] == -1.0).all() and mp[1] < 1e-14 and mp[1] != -1.0
    assert_well_formed(cov[[0, 2]], st[[0, 2]], mp[[0, 2]])
    check_against_ref(oracle, b, pose, res, cov, st, mp)


def _position_sigma_mm(cov, sigma=0.5):
    """1 sigma of the camera position (the top-left 3x3 block: the centre is -t_c) at pixel noise
    sigma, sqrt of the block's trace, in mm."""
    return 1e3 * sigma * np.sqrt(np.einsum("qii->q", cov[:, :3, :3]))


def test_under_cauchy_on_shifted_queries(lm, oracle, clean96, shifted96):
    loc = lm.Localizer(shifted96, loss=(lm.LOSS_CAUCHY, 3.0))
    pose, res, _ = loc.solve()
    assert (res["status"] == 0).all()
    cov, st, mp = loc.covariance()
    assert_well_formed(cov, st, mp)
    check_against_ref(oracle, shifted96, pose, res, cov, st, mp, loss_ref.CAUCHY, 3.0)
    locc = lm.Localizer(clean96)
    locc.solve()
    covc, stc, _ = locc.covariance()
    assert (stc == lm.COV_OK).all()
    print(f"median 1 sigma of the camera position at 0.5 px: clean batch without a loss "
          f"{np.median(_position_sigma_mm(covc)):.2f} mm, shifted batch under Cauchy(3 px) "
          f"{np.median(_position_sigma_mm(cov)):.2f} mm")


def test_state(lm, oracle, shifted96):
    cauchy = (lm.LOSS_CAUCHY, 3.0)
    loc = lm.Localizer(shifted96, loss=cauchy)
    with pytest.raises(lm.LMError) as e:                      # loaded, not solved
        loc.covariance()
    assert e.value.code == -7
    pose, res, _ = loc.solve()
    a = loc.covariance()
    b = loc.covariance()
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    # reading the covariance changes nothing a solve returns
    pose2, res2, _ = loc.solve()
    fresh_pose, fresh_res, _ = lm.Localizer(shifted96, loss=cauchy).solve()
    for p, r in ((pose, res), (pose2, res2)):
        np.testing.assert_array_equal(p, fresh_pose)
        for f in RESULT_FIELDS:
            np.testing.assert_array_equal(r[f], fresh_res[f], err_msg=f)
    # a new default loss does not reach the covariance before the next solve
    loc.set_loss(lm.LOSS_NONE)
    c = loc.covariance()
    for x, y in zip(a, c):
        np.testing.assert_array_equal(x, y)
    check_against_ref(oracle, shifted96, pose, res, *c, loss_ref.CAUCHY, 3.0)
    loc.solve()
    d = loc.covariance()
    assert np.abs(d[0] / a[0] - 1.0).max() > 1e-3
    # a reload needs a new solve
    with pytest.raises(lm.LMError) as e:
        lm.Localizer(shifted96).covariance()
    assert e.value.code == -7


def test_one_shot_equals_resident(lm, shifted96):
    for loss in (None, (lm.LOSS_CAUCHY, 3.0)):
        loc = lm.Localizer(shifted96, loss=loss)
        pose, res, _ = loc.solve()
        cov, st, _ = loc.covariance()
        p1, r1, c1, s1 = lm.localize_many(shifted96, loss=loss, covariance=True)
        np.testing.assert_array_equal(p1, pose)
        np.testing.assert_array_equal(c1, cov)
        np.testing.assert_array_equal(s1, st)
        p0, r0 = lm.localize_many(shifted96, loss=loss)
        np.testing.assert_array_equal(p0, pose)
        for f in RESULT_FIELDS:
            np.testing.assert_array_equal(r1[f], res[f], err_msg=f)
            np.testing.assert_array_equal(r0[f], res[f], err_msg=f)


def test_slam_mirror_covariance(lm, oracle):
    """cfg1 mapped from its first two captures, the third localized (as test_gpu_slam.py does):
    its covariance matches the reference at the mirror's pose; a mapping capture answers STATE."""
    g = synth.config_graph("cfg1")
    s = lm.SlamSolver()
    try:
        s.set_camera(g.camera)
        for c in range(3):
            if c == 2:
                s.solve()
                first = s.num_captures
            sel = g.obs_cap == c
            s.add_detections(f"cap{c}", [f"tag_{t}" for t in g.obs_tag[sel]], g.corners[sel])
        with pytest.raises(lm.LMError) as e:                  # no localize_many yet
            s.localize_covariance(first)
        assert e.value.code == -7
        s.localize_many(first)
        pose_before = s.capture_poses().copy()
        cov, st = s.localize_covariance(first)
        cov2, st2 = s.localize_covariance(first)
        np.testing.assert_array_equal(cov, cov2)
        np.testing.assert_array_equal(s.capture_poses(), pose_before)
        for c in range(first):
            with pytest.raises(lm.LMError) as e:
                s.localize_covariance(c)
            assert e.value.code == -7
        in_map = np.zeros(s.num_arucos, np.uint8)
        obs_tag, corners = [], []
        for b in range(s.num_blocks):
            c, a, rect, _ = s.block(b)
            if c < first:
                in_map[a] = 1
            else:
                obs_tag.append(a)
                corners.append(rect)
        batch = synth.LocalizeBatch(s.camera()[0], s.aruco_poses(), np.array([0, len(obs_tag)], np.int32),
                                    np.array(obs_tag, np.int32), np.array(corners), None, in_map)
        pose = s.capture_poses()[first:first + 1].copy()
    finally:
        s.close()
    assert st == lm.COV_OK
    p1, r1, c1, s1 = lm.localize_many(batch, covariance=True)
    np.testing.assert_array_equal(p1, pose)                   # the mirror's poses are localize_many's
    np.testing.assert_array_equal(c1[0], cov)
    check_against_ref(oracle, batch, pose, r1, cov[None], np.array([st]), None, parity=False)


def test_covariance_predicts_the_pose_error_on_the_device(lm, oracle):
    """N = 2048 noisy copies of one query (the first 2048 of the CPU test's): m = mean
    d' (sigma^2 C_q)^-1 d = 6 within 5 sqrt(12 / 2048) = 0.38 (a factor of two in C, or the t and w
    blocks swapped, gives 3, 12 or worse); every term agrees with the reference's to 1e-6."""
    n = 2048
    assert n <= STAT_N
    b = stat_batch(n)
    loc = lm.Localizer(b)
    pose, res, _ = loc.solve()
    assert (res["status"] == 0).all()
    cov, st, mp = loc.covariance()
    assert (st == lm.COV_OK).all()
    terms = cov_ref.chi2_terms(cov, pose, b.pose_true, SIGMA)
    m = terms.mean()
    print(f"N = {n}: m = {m:.3f} (bound 6 +- {5 * np.sqrt(12.0 / n):.2f})")
    assert abs(m - 6.0) <= 5.0 * np.sqrt(12.0 / n)
    c_ref, s_ref, _ = cov_ref.covariance(oracle, b, pose, status=res["status"], rule=res["rule"])
    assert (s_ref == cov_ref.OK).all()
    t_ref = cov_ref.chi2_terms(c_ref, pose, b.pose_true, SIGMA)
    print("terms against the reference's:", np.abs(terms / t_ref - 1.0).max())
    np.testing.assert_allclose(terms, t_ref, rtol=1e-6)
