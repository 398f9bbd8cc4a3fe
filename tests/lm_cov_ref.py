"""numpy reference of the LM solver's marginal covariances (test helper, no GPU).

The definition arslam_lm_covariance is held to (include/arslam_lm.h): at given parameters,
H = J~'J~ over every observation and every free parameter -- the focal if the camera is free
(never l1, l2), 6 per free capture, 6 per free tag; a block is free when it is not constant and
some observation uses it -- with the rows corrected by sqrt(rho') (tests/loss_ref.py).  C = H^-1;
the marginals are its 6x6 diagonal blocks and var(f).

C is computed by two routes on the Jacobi-scaled Jacobian Js = J s:
  route 1  inv(Js'Js), unscaled -- the normal equations, what the device solves;
  route 2  QR of Js, C = s R^-1 R^-T s -- never squares the condition number.
The reference is route 2; e_ref, the largest disagreement of the two on the marginal blocks
relative to sqrt(C_ii C_jj), measures the error class of route 1 on that input.

Also the tile recursion of the device's selected inverse (selinv.hip), restated on a dense
numpy Cholesky factor with the same right-hand-side masking.
"""
import numpy as np

import loss_ref

OK, UNAVAILABLE, RANK_DEFICIENT = 0, 1, 2
TILE = 64


class CovRef:
    """cap (nc, 6, 6), tag (nt, 6, 6): the marginal blocks (-1 where the block is not free);
    var_f (-1 likewise); cap_status / tag_status; e_ref; min_pivot; cols: the free parameters'
    indices in [camera 3 | captures 6 nc | tags 6 nt]; C: the whole covariance over cols."""


def jacobi_scale(J):
    """Ceres' Jacobian scaling 1 / (1 + sqrt(squared column norm)) of the dense J."""
    return 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))


def free_columns(arrays, camera_const=False, cap_const=None, tag_const=None):
    """(cols, cap_free, tag_free, cam_free) of a (camera, cap, tag, obs_cap, obs_tag, corners) problem."""
    _, cap, tag, obs_cap, obs_tag, _ = arrays
    nc, nt = len(cap), len(tag)
    cap_const = np.zeros(nc, bool) if cap_const is None else np.asarray(cap_const, bool)
    tag_const = np.zeros(nt, bool) if tag_const is None else np.asarray(tag_const, bool)
    cap_free = ~cap_const & (np.bincount(obs_cap, minlength=nc) > 0)
    tag_free = ~tag_const & (np.bincount(obs_tag, minlength=nt) > 0)
    # an observation is active when one of its blocks is free; the camera is used by an active one
    active = (not camera_const) | cap_free[obs_cap] | tag_free[obs_tag]
    cam_free = (not camera_const) and bool(np.any(active))
    cols = ([0] if cam_free else []) + [3 + 6 * c + i for c in np.nonzero(cap_free)[0] for i in range(6)] + \
        [3 + 6 * nc + 6 * t + i for t in np.nonzero(tag_free)[0] for i in range(6)]
    return np.array(cols, np.int64), cap_free, tag_free, cam_free


def covariance(oracle, arrays, camera_const=False, cap_const=None, tag_const=None, kinds=0, a=0.0,
               scale_arrays=None, rows=None):
    """The marginal covariances of the problem `arrays` = (camera, cap, tag, obs_cap, obs_tag,
    corners) at its parameters.  scale_arrays: the parameters at which the Jacobi scale is taken
    (the device keeps the scale of its solve's first linearization; None: the same parameters).
    min_pivot: the smallest squared Cholesky pivot of the scaled H over the reduced rows when the
    captures are eliminated first and the tags, then the focal, follow in index order -- the
    pivots of the reduced system in that order.  rows = (cap_row, tag_row, cam_row): the device's
    reduced rows (lm.debug_reduced_rows); min_pivot_rows is then the same figure with the blocks of
    row -1 eliminated first and the others in the device's row order (what the device reports)."""
    camera, cap, tag, obs_cap, obs_tag, corners = arrays
    cap = np.asarray(cap, np.float64).reshape(-1, 6)
    tag = np.asarray(tag, np.float64).reshape(-1, 6)
    obs_cap, obs_tag = np.asarray(obs_cap), np.asarray(obs_tag)
    arrays = (camera, cap, tag, obs_cap, obs_tag, corners)
    nc, nt = len(cap), len(tag)
    cols, cap_free, tag_free, cam_free = free_columns(arrays, camera_const, cap_const, tag_const)
    J = loss_ref.robust_terms(oracle, arrays, kinds, a).dense_jacobian()[:, cols]
    if scale_arrays is None:
        s = jacobi_scale(J)
    else:
        s = jacobi_scale(loss_ref.robust_terms(oracle, scale_arrays, kinds, a).dense_jacobian()[:, cols])
    Js = J * s
    Hs = Js.T @ Js
    C1 = np.linalg.inv(Hs) * np.outer(s, s)
    R = np.linalg.qr(Js, mode="r")
    Ri = np.linalg.solve(R, np.eye(len(cols)))   # (R is upper triangular)
    C2 = (Ri @ Ri.T) * np.outer(s, s)
    C2 = 0.5 * (C2 + C2.T)
    ref = CovRef()
    ref.cols, ref.C = cols, C2
    pos = {int(c): i for i, c in enumerate(cols)}
    ref.cap = -np.ones((nc, 6, 6))
    ref.tag = -np.ones((nt, 6, 6))
    ref.cap_status = np.where(cap_free, OK, UNAVAILABLE)
    ref.tag_status = np.where(tag_free, OK, UNAVAILABLE)
    ref.var_f = float(C2[0, 0]) if cam_free else -1.0
    e = abs(C1[0, 0] - C2[0, 0]) / C2[0, 0] if cam_free else 0.0
    for free, first, out in ((cap_free, 3, ref.cap), (tag_free, 3 + 6 * nc, ref.tag)):
        for b in np.nonzero(free)[0]:
            i0 = pos[first + 6 * int(b)]
            sl = slice(i0, i0 + 6)
            out[b] = C2[sl, sl]
            d = np.sqrt(np.diag(C2[sl, sl]))
            e = max(e, float(np.max(np.abs(C1[sl, sl] - C2[sl, sl]) / np.outer(d, d))))
    ref.e_ref = float(e)
    # the reduced system's pivots: Cholesky of the scaled H with the eliminated blocks first
    nat = (-np.ones(nc, np.int64), np.where(tag_free, 6 * np.arange(nt), -1), 6 * nt if cam_free else -1)

    def min_pivot(cap_row, tag_row, cam_row):
        key = np.zeros(len(cols))
        for i, c in enumerate(cols):
            if c == 0:
                key[i] = cam_row
            elif c < 3 + 6 * nc:
                r = cap_row[(c - 3) // 6]
                key[i] = r + (c - 3) % 6 if r >= 0 else -1
            else:
                r = tag_row[(c - 3 - 6 * nc) // 6]
                key[i] = r + (c - 3 - 6 * nc) % 6 if r >= 0 else -1
        order = np.argsort(key, kind="stable")
        L = np.linalg.cholesky(Hs[np.ix_(order, order)])
        piv = np.diag(L)[key[order] >= 0] ** 2
        return float(piv.min()) if len(piv) else 1.0

    ref.min_pivot = min_pivot(*nat)
    ref.min_pivot_rows = min_pivot(*rows) if rows is not None else ref.min_pivot
    return ref


def graph_arrays(g, camera=None, cap=None, tag=None):
    return (g.camera if camera is None else camera, g.cap if cap is None else cap, g.tag if tag is None else tag,
            g.obs_cap, g.obs_tag, g.corners)


# ---- the selected inverse's tile recursion ----

def tile_fill(pattern):
    """Symbolic tile Cholesky fill of a lower (T, T) pattern (diagonal included)."""
    P = np.tril(np.asarray(pattern) != 0)
    T = P.shape[0]
    P[np.arange(T), np.arange(T)] = True
    for k in range(T):
        rows = [i for i in range(k + 1, T) if P[i, k]]
        for x in rows:
            for y in rows:
                if y <= x:
                    P[x, y] = True
    return P


def tile_selinv(A, pattern=None):
    """Z = A^-1 on the tiles of A's factor by the recursion of selinv.hip, in numpy.

    A (n, n) SPD; pattern: None (dense) or the lower (T, T) tile pattern A is restricted to, T =
    (n + 1 + 63) // 64.  As on the device the matrix is padded to N = 64 T with a right-hand-side
    row n (pivot 1e300) and identity rows after it; with r0 = n - 64 (n // 64), rows >= r0 of every
    G tile in tile row n // 64 and rows and columns >= r0 of that tile's X_kk are zeroed.
    Returns (Z (n, n), 0 off the filled pattern; the filled lower pattern (T, T))."""
    n = A.shape[0]
    T = (n + 1 + TILE - 1) // TILE
    N = T * TILE
    P0 = np.tril(np.ones((T, T), bool)) if pattern is None else np.tril(np.asarray(pattern) != 0)
    P0[np.arange(T), np.arange(T)] = True
    M = np.zeros((N, N))
    M[:n, :n] = A
    M *= np.kron(P0 | P0.T, np.ones((TILE, TILE)))
    M[n, n] = 1e300
    M[np.arange(n + 1, N), np.arange(n + 1, N)] = 1.0
    P = tile_fill(P0)
    L = np.linalg.cholesky(M)

    def t(X, i, j):
        return X[TILE * i:TILE * (i + 1), TILE * j:TILE * (j + 1)]

    kr, r0 = n // TILE, n - TILE * (n // TILE)
    X = [np.linalg.inv(t(L, k, k)) for k in range(T)]
    X[kr][r0:, :] = 0.0
    X[kr][:, r0:] = 0.0
    G = {}
    for k in range(T):
        for j in range(k + 1, T):
            if P[j, k]:
                G[j, k] = t(L, j, k) @ X[k]
                if j == kr:
                    G[j, k][r0:, :] = 0.0
    Z = np.zeros((N, N))
    for k in range(T - 1, -1, -1):   # root first: a column's ancestors have larger indices
        I = [j for j in range(k + 1, T) if P[j, k]]
        for i in I:
            acc = np.zeros((TILE, TILE))
            for j in I:
                Zij = t(Z, i, j) if i >= j else t(Z, j, i).T
                acc += Zij @ G[j, k]
            t(Z, i, k)[:] = -acc
        acc = X[k].T @ X[k]
        for j in I:
            acc = acc - G[j, k].T @ t(Z, j, k)
        low = np.tril(acc)
        t(Z, k, k)[:] = low + np.tril(low, -1).T
    Zl = np.tril(Z)
    Zs = Zl + np.tril(Zl, -1).T
    Zs *= np.kron(P | P.T, np.ones((TILE, TILE)))
    return Zs[:n, :n], P
