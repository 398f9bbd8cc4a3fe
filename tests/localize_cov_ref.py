"""numpy reference of the batched localizer's per-query pose covariance (test helper, no GPU).

Restates the definition of include/arslam_localize.h over localize_ref._Query.terms: at a given
pose, H = J~'J~ with the rows scaled by sqrt(rho'(s)) per observation (no LM diagonal, no Jacobi
scaling); c_j = 1/sqrt(H_jj), Hs = c H c with a unit diagonal, Cholesky Hs = L L',
C = c (L^-T L^-1) c; min_pivot = min_j L_jj^2; a query is rank deficient when some H_jj is not
finite and > 0 or some squared pivot is not >= 1e-14.
"""
import numpy as np

import localize_ref

OK, UNAVAILABLE, RANK_DEFICIENT = 0, 1, 2
MIN_PIVOT = 1e-14
RULE_EVAL_FAILED = localize_ref.RULE_EVAL_FAILED


def normal_matrix(qr, x):
    """(finite, H = J~'J~ (6, 6)) of one query (localize_ref._Query) at the pose x."""
    s, rho, rho1, r, J = qr.terms(np.asarray(x, np.float64))
    Jt = (np.sqrt(rho1)[:, None, None] * J).reshape(-1, 6)
    finite = bool(np.isfinite(r).all() and np.isfinite(rho).all())
    return finite, Jt.T @ Jt


def invert(H):
    """(cov (6, 6), status, min_pivot) of one normal matrix by the equilibrated Cholesky."""
    bad = np.full((6, 6), -1.0)
    d = np.diag(H)
    if not (np.isfinite(d) & (d > 0.0)).all():
        return bad, RANK_DEFICIENT, -1.0
    c = 1.0 / np.sqrt(d)
    Hs = c[:, None] * H * c[None, :]
    np.fill_diagonal(Hs, 1.0)
    L = np.zeros((6, 6))
    pivots = np.zeros(6)
    for j in range(6):
        s = Hs[j, j] - L[j, :j] @ L[j, :j]
        pivots[j] = s
        if not s >= MIN_PIVOT:          # (a negative or NaN pivot included)
            return bad, RANK_DEFICIENT, float(s)
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 6):
            L[i, j] = (Hs[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    Li = np.linalg.solve(L, np.eye(6))
    Cm = c[:, None] * (Li.T @ Li) * c[None, :]
    Cm = np.triu(Cm) + np.triu(Cm, 1).T          # one triangle, mirrored
    return Cm, OK, float(pivots.min())


def covariance(oracle, batch, pose, kinds=None, scales=None, status=None, rule=None):
    """Per query the covariance at pose[q] (n_query, 6), its status and min_pivot.  status /
    rule: the solve's, per query (SKIPPED, or FAILURE with rule EVAL_FAILED -> UNAVAILABLE)."""
    nq = batch.n_query
    cov, st, mp = np.full((nq, 6, 6), -1.0), np.full(nq, UNAVAILABLE, np.int32), np.full(nq, -1.0)
    for q, a, b, qr in localize_ref._queries(oracle, batch, kinds, scales):
        if b == a or (status is not None and status[q] == localize_ref.SKIPPED):
            continue
        if status is not None and rule is not None and status[q] == localize_ref.FAILURE \
                and rule[q] == RULE_EVAL_FAILED:
            continue
        finite, H = normal_matrix(qr, pose[q])
        if not finite:
            continue
        cov[q], st[q], mp[q] = invert(H)
    return cov, st, mp


def chi2_terms(cov, pose, pose_true, sigma):
    """d' (sigma^2 C_q)^-1 d per query, d = pose - pose_true."""
    d = np.asarray(pose) - np.asarray(pose_true)
    return np.array([d[q] @ np.linalg.solve(sigma * sigma * cov[q], d[q]) for q in range(len(d))])


def replicated_batch(base, q, n, sigma, seed):
    """Query q of `base` (a noise-free batch) n times, with independent N(0, sigma) noise on every
    corner coordinate; pose_true = the query's true pose."""
    from ar_slam_amd import synth
    rng = np.random.default_rng(seed)
    a, b = int(base.q_start[q]), int(base.q_start[q + 1])
    k = b - a
    corners = np.tile(np.asarray(base.corners, np.float64).reshape(-1, 8)[a:b], (n, 1))
    corners = corners + rng.normal(0.0, sigma, corners.shape)
    return synth.LocalizeBatch(base.camera, base.tag, (k * np.arange(n + 1)).astype(np.int32),
                               np.tile(base.obs_tag[a:b], n).astype(np.int32), corners,
                               np.tile(base.pose_true[q], (n, 1)), base.tag_in_map.copy())
