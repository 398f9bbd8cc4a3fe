"""numpy reference of the LM solver's cross-covariance blocks (test helper, no GPU).

arslam_lm_covariance_pairs (include/arslam_lm.h) returns blocks of the same matrix C = H^-1 that
tests/lm_cov_ref.py defines: block (a, b) is cut out of CovRef.C over CovRef.cols, in the SoA
layout of the header (rows of a by columns of b; the focal against a pose: cov(f, pose) in the
first six values; camera against camera: var(f) at [0]).  e_ref_pairs is lm_cov_ref's
route-1-vs-route-2 disagreement, inv(Js'Js) against QR, over the requested blocks, relative to
sqrt(C_ii C_jj), i in a and j in b.

Also the device's multi-right-hand-side tile solve (cov_pairs.hip), restated on a dense numpy
Cholesky factor with the same right-hand-side masking, and the pair lists the tests use.
"""
import numpy as np

import lm_cov_ref as cov_ref
import loss_ref

OK, UNAVAILABLE, RANK_DEFICIENT = cov_ref.OK, cov_ref.UNAVAILABLE, cov_ref.RANK_DEFICIENT
CAMERA, CAPTURE, TAG = 0, 1, 2     # arslam_lm.h ARSLAM_BLOCK_*
TILE = cov_ref.TILE
PANEL_BLOCKS = 10                  # 6-column blocks per 64-column panel (cov_pairs.hip)


class PairsRef:
    """cov (n, 6, 6), status (n,), e_ref_pairs, joint: per pair the reference's 12x12 (or smaller)
    joint matrix of the two blocks' free parameters (None unless OK); ref: the CovRef behind it."""


def _block_cols(ref, nc, kind, index):
    """Positions in ref.cols of a block's free parameters (the focal alone for the camera), or None."""
    first = 0 if kind == CAMERA else 3 + 6 * index if kind == CAPTURE else 3 + 6 * nc + 6 * index
    pos = np.nonzero(ref.cols == first)[0]
    if len(pos) == 0:
        return None
    return np.arange(pos[0], pos[0] + (1 if kind == CAMERA else 6))


def cut(C, ia, ib):
    """Block (a, b) of C in the SoA layout: 6x6 with the focal's values first."""
    out = np.zeros(36)
    out[:len(ia) * len(ib)] = C[np.ix_(ia, ib)].ravel()
    return out.reshape(6, 6)


def covariance_pairs(oracle, arrays, pairs, camera_const=False, cap_const=None, tag_const=None, kinds=0, a=0.0,
                     scale_arrays=None, rows=None):
    """The blocks `pairs` = [((kind_a, index_a), (kind_b, index_b)), ...] of the reference covariance
    (lm_cov_ref.covariance with the same arguments)."""
    ref = cov_ref.covariance(oracle, arrays, camera_const, cap_const, tag_const, kinds, a, scale_arrays, rows)
    nc = len(np.asarray(arrays[1]).reshape(-1, 6))
    # route 1 over the same columns and scale: the normal equations' inverse
    J = loss_ref.robust_terms(oracle, arrays, kinds, a).dense_jacobian()[:, ref.cols]
    s = cov_ref.jacobi_scale(J if scale_arrays is None else
                             loss_ref.robust_terms(oracle, scale_arrays, kinds, a).dense_jacobian()[:, ref.cols])
    Js = J * s
    C1 = np.linalg.inv(Js.T @ Js) * np.outer(s, s)
    d = np.sqrt(np.diag(ref.C))
    out = PairsRef()
    out.ref = ref
    out.cov = -np.ones((len(pairs), 6, 6))
    out.status = np.full(len(pairs), UNAVAILABLE)
    out.joint = [None] * len(pairs)
    out.scale = [None] * len(pairs)   # sqrt(C_ii C_jj) in the layout of cov
    e = 0.0
    for p, (ba, bb) in enumerate(pairs):
        ia, ib = _block_cols(ref, nc, *ba), _block_cols(ref, nc, *bb)
        if ia is None or ib is None:
            continue
        out.status[p] = OK
        out.cov[p] = cut(ref.C, ia, ib)
        sc = np.ones(36)
        sc[:len(ia) * len(ib)] = np.outer(d[ia], d[ib]).ravel()
        out.scale[p] = sc.reshape(6, 6)
        e = max(e, float(np.max(np.abs(C1[np.ix_(ia, ib)] - ref.C[np.ix_(ia, ib)]) / np.outer(d[ia], d[ib]))))
        both = np.concatenate([ia, ib]) if not np.array_equal(ia, ib) else ia
        out.joint[p] = ref.C[np.ix_(both, both)]
    out.e_ref_pairs = e
    return out


def joint_from_blocks(caa, cab, cba, cbb, fa=False, fb=False):
    """[[C_aa, C_ab], [C_ba, C_bb]] from blocks in the SoA layout (fa / fb: the block is the focal)."""
    na, nb = (1 if fa else 6), (1 if fb else 6)

    def blk(c, r, q):
        return np.asarray(c).ravel()[:r * q].reshape(r, q)
    return np.block([[blk(caa, na, na), blk(cab, na, nb)], [blk(cba, nb, na), blk(cbb, nb, nb)]])


# ---- the pair lists ----

def pair_list(inp):
    """The parity pair list of a CovInput and, by category, what it holds.  Categories a graph cannot
    supply (two captures sharing no tag on a graph where all do) are absent from the dict."""
    g = inp.g
    cc, tc = inp.consts()
    nc, nt = g.n_cap, g.n_tag
    sees = np.zeros((nc, nt), bool)
    sees[g.obs_cap, g.obs_tag] = True
    caps = [c for c in range(nc) if not cc[c] and sees[c].any()]
    tags = [t for t in range(nt) if not tc[t] and sees[:, t].any()]
    cam = not inp.camera_const
    cat = {}
    pos = g.tag_true[:, :3]
    dist = np.linalg.norm(pos[tags][:, None] - pos[tags][None], axis=2)
    i, j = np.unravel_index(np.argmax(dist), dist.shape)
    cat["tag_tag_far"] = ((TAG, tags[i]), (TAG, tags[j]))
    np.fill_diagonal(dist, np.inf)
    i, j = np.unravel_index(np.argmin(dist), dist.shape)
    cat["tag_tag_adjacent"] = ((TAG, tags[i]), (TAG, tags[j]))
    shared = (sees[caps].astype(int) @ sees[caps].T.astype(int))
    for name, want in (("cap_cap_sharing", True), ("cap_cap_disjoint", False)):
        for x in range(len(caps)):
            ys = [y for y in range(x + 1, len(caps)) if (shared[x, y] > 0) == want]
            if ys:
                cat[name] = ((CAPTURE, caps[x]), (CAPTURE, caps[ys[-1]]))
                break
    for name, want in (("cap_tag_seen", True), ("cap_tag_unseen", False)):
        for c in caps[::-1]:
            ts = [t for t in tags if sees[c, t] == want]
            if ts:
                cat[name] = ((CAPTURE, c), (TAG, ts[len(ts) // 2]))
                break
    if cam:
        cat["camera_tag"] = ((CAMERA, 0), (TAG, tags[len(tags) // 2]))
        cat["camera_capture"] = ((CAPTURE, caps[len(caps) // 2]), (CAMERA, 0))
        cat["camera_camera"] = ((CAMERA, 0), (CAMERA, 0))
    cat["tag_self"] = ((TAG, tags[-1]), (TAG, tags[-1]))
    cat["cap_self"] = ((CAPTURE, caps[-1]), (CAPTURE, caps[-1]))
    a, b = cat["cap_tag_seen"]
    cat["reversed"] = (b, a)
    cat["duplicate"] = cat["tag_tag_far"]
    pairs = list(cat.values())
    # chains of neighbours in index order: at least 11 distinct solved blocks, two panels
    chain = [((TAG, x), (TAG, y)) for x, y in zip(tags[:13], tags[1:14])]
    if len(chain) < 11:
        chain += [((CAPTURE, x), (CAPTURE, y)) for x, y in zip(caps[:13], caps[1:14])]
    return pairs + chain, cat


def solved_blocks(pairs, tags_eliminated):
    """The distinct right-hand blocks of a pair list by the device's rule (lm_covariance.hip): of
    each unordered pair the block of the smaller key -- the focal, then the reduced side's blocks
    by index, then the eliminated side's."""
    def key(b):
        kind, idx = b
        if kind == CAMERA:
            return (0, 0)
        return (2 if (kind == TAG) == tags_eliminated else 1, idx)
    return {min(key(a), key(b)) for a, b in pairs}


# ---- the tile solve ----

def tile_solve(A, B, pattern=None):
    """X = A^-1 B by the forward and backward tile recursion of cov_pairs.hip, in numpy.

    A (n, n) SPD, pattern as in lm_cov_ref.tile_selinv; B (n, nrhs).  The matrix is padded to N =
    64 T with a right-hand-side row n (pivot 1e300) and identity rows after it; rows >= n of every
    factor tile and rows and columns >= n of every L_kk^-1 are read as zero, so the padded rows of
    X stay zero."""
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
    P = cov_ref.tile_fill(P0)
    L = np.linalg.cholesky(M)

    def t(X, i, j):
        return X[TILE * i:TILE * (i + 1), TILE * j:TILE * (j + 1)]

    def lim(k):
        return int(np.clip(n - TILE * k, 0, TILE))

    Li, Lo = [], {}
    for k in range(T):
        X = np.linalg.inv(t(L, k, k))
        X[lim(k):, :] = 0.0
        X[:, lim(k):] = 0.0
        Li.append(X)
        for j in range(k):
            if P[k, j]:
                Lo[k, j] = t(L, k, j).copy()
                Lo[k, j][lim(k):, :] = 0.0
    Y = np.zeros((N, B.shape[1]))
    Y[:n] = B
    for k in range(T):                 # a tile row's descendants have smaller indices
        acc = np.zeros((TILE, B.shape[1]))
        for j in range(k):
            if P[k, j]:
                acc += Lo[k, j] @ Y[TILE * j:TILE * (j + 1)]
        Y[TILE * k:TILE * (k + 1)] = Li[k] @ (Y[TILE * k:TILE * (k + 1)] - acc)
    for k in range(T - 1, -1, -1):     # root first
        acc = np.zeros((TILE, B.shape[1]))
        for j in range(k + 1, T):
            if P[j, k]:
                acc += Lo[j, k].T @ Y[TILE * j:TILE * (j + 1)]
        Y[TILE * k:TILE * (k + 1)] = Li[k].T @ (Y[TILE * k:TILE * (k + 1)] - acc)
    assert np.all(Y[n:] == 0.0)
    return Y[:n]


def solve_columns(n, nrhs):
    """Identity columns for the solve tests: both ends and across every tile boundary."""
    want = [0, n - 1]
    for b in range(TILE, n, TILE):
        want += [b - 1, b]
    want += list(np.linspace(0, n - 1, nrhs).astype(int))
    cols = []
    for c in want:
        if 0 <= c < n and c not in cols:
            cols.append(int(c))
    k = 0
    while len(cols) < nrhs:            # (nrhs > n: columns repeat)
        cols.append(k % n)
        k += 1
    return np.array(cols[:nrhs])
