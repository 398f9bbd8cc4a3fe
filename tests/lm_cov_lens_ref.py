"""numpy reference of the covariance with the lens estimated (test helper, no GPU).

lm_cov_ref.covariance over the camera columns [f, l1, l2]: the definition
arslam_lm_covariance_lens and arslam_lm_covariance_pairs_lens are held to (include/arslam_lm.h).
H = J~'J~ over every free parameter, l1 and l2 among them when the camera is free and `lens` is
set; the oracle is distortion_free_ref.FreeRadialOracle (whose Jacobian has the two l columns),
alone or inside tag_size_ref.SizedOracle, and the rows are corrected by loss_ref as everywhere.
The same two routes (the inverse of the scaled normal equations, and QR); the reference is the QR
route, and e_ref -- their largest disagreement relative to sqrt(C_ii C_jj) -- runs over the
camera's 3x3 too.  With lens=False the l columns are dropped and every figure is
lm_cov_ref.covariance's over distortion_ref.RadialOracle, exactly.

min_pivot in the device's row order: the camera's rows are cam_row, cam_row + 1, cam_row + 2.
"""
import numpy as np

import lm_cov_ref
import loss_ref
from lm_cov_ref import OK, UNAVAILABLE, RANK_DEFICIENT, jacobi_scale   # noqa: F401

CAMERA, CAPTURE, TAG = 0, 1, 2    # arslam_lm.h ARSLAM_BLOCK_*


class LensCovRef:
    """cam (3, 3) (held l1, l2: their rows and columns 0; -1 everywhere for a camera that is not
    free), cam_status; cap, tag, cap_status, tag_status, var_f, e_ref, min_pivot (captures
    eliminated first), min_pivot_tags (tags first), min_pivot_rows, cols, C as lm_cov_ref.CovRef;
    n_cam: the camera's columns in cols (0, 1 or 3); nc."""

    def block_cols(self, kind, index):
        """The positions in cols / C of a block's parameters ([] for one that is not free)."""
        if kind == CAMERA:
            return list(range(self.n_cam))
        first = 3 + 6 * index if kind == CAPTURE else 3 + 6 * self.nc + 6 * index
        pos = np.nonzero(self.cols == first)[0]
        return list(range(int(pos[0]), int(pos[0]) + 6)) if len(pos) else []

    def pair(self, a, b):
        """Block (a, b) in arslam_lm_covariance_pairs_lens' layout: (6, 6), the camera's rows (as a)
        or columns (as b) its first 1 or 3, the rest 0; None when either block is not free."""
        ia, ib = self.block_cols(*a), self.block_cols(*b)
        if not ia or not ib:
            return None
        out = np.zeros((6, 6))
        out[:len(ia), :len(ib)] = self.C[np.ix_(ia, ib)]
        return out


def covariance(oracle, arrays, camera_const=False, cap_const=None, tag_const=None, kinds=0, a=0.0,
               scale_arrays=None, rows=None, lens=True):
    """lm_cov_ref.covariance's arguments; lens: l1, l2 are parameters of a free camera."""
    camera, cap, tag, obs_cap, obs_tag, corners = arrays
    cap = np.asarray(cap, np.float64).reshape(-1, 6)
    tag = np.asarray(tag, np.float64).reshape(-1, 6)
    obs_cap, obs_tag = np.asarray(obs_cap), np.asarray(obs_tag)
    arrays = (camera, cap, tag, obs_cap, obs_tag, corners)
    nc, nt = len(cap), len(tag)
    cols, cap_free, tag_free, cam_free = lm_cov_ref.free_columns(arrays, camera_const, cap_const, tag_const)
    n_cam = (3 if lens else 1) if cam_free else 0
    if n_cam == 3:
        cols = np.concatenate([[0, 1, 2], cols[1:]]).astype(np.int64)
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
    ref = LensCovRef()
    ref.cols, ref.C, ref.n_cam, ref.nc = cols, C2, n_cam, nc
    pos = {int(c): i for i, c in enumerate(cols)}
    ref.cap = -np.ones((nc, 6, 6))
    ref.tag = -np.ones((nt, 6, 6))
    ref.cap_status = np.where(cap_free, OK, UNAVAILABLE)
    ref.tag_status = np.where(tag_free, OK, UNAVAILABLE)
    ref.var_f = float(C2[0, 0]) if cam_free else -1.0
    ref.cam_status = OK if cam_free else UNAVAILABLE
    ref.cam = np.zeros((3, 3)) if cam_free else -np.ones((3, 3))
    e = 0.0
    if cam_free:
        ref.cam[:n_cam, :n_cam] = C2[:n_cam, :n_cam]
        dd = np.diag(C2)[:n_cam]
        e = float(np.max(np.abs(C1[:n_cam, :n_cam] - C2[:n_cam, :n_cam]) / np.sqrt(np.outer(dd, dd))))
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
    swp = (np.where(cap_free, 6 * np.arange(nc), -1), -np.ones(nt, np.int64), 6 * nc if cam_free else -1)

    def min_pivot(cap_row, tag_row, cam_row):
        key = np.zeros(len(cols))
        for i, c in enumerate(cols):
            if c < 3:
                key[i] = cam_row + c
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
    ref.min_pivot_tags = min_pivot(*swp)
    ref.min_pivot_rows = min_pivot(*rows) if rows is not None else ref.min_pivot
    return ref
