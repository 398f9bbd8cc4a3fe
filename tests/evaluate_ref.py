"""numpy reference of arslam_lm_evaluate (test helper, no GPU).

ceres::Problem::Evaluate (Ceres 2.0, default EvaluateOptions) over the oracle's residuals and
Jacobians: loss_ref.RobustTerms, through tag_size_ref.SizedOracle for per-tag sides and
distortion_ref.RadialOracle / distortion_free_ref.FreeRadialOracle for the lens.  The gradient's
entries of constant blocks, of blocks no observation touches and of the lens parameters that are
not estimated are zeroed, as the device leaves them.

Tolerances.  The residuals: the project's row bound, rtol = 1e-12, atol = 1e-9
(tests/test_gpu_parity.py).  Every other quantity q(r, J) gets that bound carried to first order,

    tol_q = sum_i |dq/dr_i| dr_i + sum_ij |dq/dJ_ij| dJ_ij,
    dr_i = 1e-12 |r_i| + 1e-9,  dJ_ij = 1e-12 max_k |J_ik|  (the Jacobian bound of the same test),

from the reference's own uncorrected r and J.  With w = rho'(s), s = sum r_i^2:

    s      ds = sum_i 2 |r_i| dr_i
    w      |rho''(s)| ds   (Huber within ds of its kink: the outer branch's rho'')
    cost   1/2 sum_o w_o ds_o
    g_j    sum_o sum_i |w J_ij + 2 rho'' r_i (J_.j . r)| dr_i + w |r_i| dJ_ij
"""
import dataclasses

import numpy as np

import distortion_free_ref
import distortion_ref
import loss_ref
import tag_size_ref

RTOL, ATOL = 1e-12, 1e-9
PINHOLE, RADIAL, RADIAL_FREE = "pinhole", "radial", "radial_free"


def rho2(kind, a, s, ds=0.0):
    """rho''(s) of loss `kind` with scale a (the larger magnitude of the two sides for a Huber
    observation within ds of the kink)."""
    b = float(a) * float(a)
    if kind == loss_ref.NONE:
        return 0.0
    if kind == loss_ref.HUBER:
        return -0.5 * a * max(s, b) ** -1.5 if s + ds > b else 0.0
    if kind == loss_ref.SOFT_L_ONE:
        return -0.5 / b * (1.0 + s / b) ** -1.5
    if kind == loss_ref.CAUCHY:
        return -1.0 / (b * (1.0 + s / b) ** 2)
    raise ValueError(kind)


def model_oracle(oracle, model):
    if model == PINHOLE:
        return oracle
    return distortion_ref.RadialOracle(oracle) if model == RADIAL else distortion_free_ref.FreeRadialOracle(oracle)


def project(oracle, arrays, model=PINHOLE, tag_size=None, noise=0.5, seed=0):
    """The problem's arrays with every observation's corners replaced by the oracle's own projection
    at the arrays' values (oracle.residual at zero corners) plus seeded Gaussian noise (px)."""
    camera, cap, tag, obs_cap, obs_tag, _ = loss_ref._arrays(arrays)
    base = model_oracle(oracle, model)
    sizes = tag_size_ref._obs_sizes(arrays, tag_size)
    rng = np.random.default_rng(seed)
    corners = np.zeros((len(obs_cap), 8))
    for o in range(len(obs_cap)):
        corners[o] = tag_size_ref.residual(base, camera, cap[obs_cap[o]], tag[obs_tag[o]], np.zeros(8), sizes[o])
    corners += noise * rng.standard_normal(corners.shape)
    return (camera, cap, tag, np.asarray(obs_cap, np.int32), np.asarray(obs_tag, np.int32), corners)


@dataclasses.dataclass
class Reference:
    cost: float
    residuals: np.ndarray
    sq_norm: np.ndarray
    weight: np.ndarray
    gradient: np.ndarray     # [camera 3 | captures 6 nc | tags 6 nt]
    zero: np.ndarray         # bool: the gradient entries that are exactly 0.0
    tol_cost: float
    tol_sq_norm: np.ndarray
    tol_weight: np.ndarray
    tol_gradient: np.ndarray

    def tol_residuals(self):
        return ATOL + RTOL * np.abs(self.residuals)


def evaluate(oracle, arrays, kinds=0, a=0.0, tag_size=None, model=PINHOLE, camera_const=False, cap_const=None,
             tag_const=None, apply_loss=True):
    """The reference of one arslam_lm_evaluate call and its tolerances."""
    camera, cap, tag, obs_cap, obs_tag, corners = loss_ref._arrays(arrays)
    nb, nc, nt = len(obs_cap), len(cap), len(tag)
    kinds = np.broadcast_to(np.asarray(kinds), (nb,)) if apply_loss else np.zeros(nb, int)
    a = np.broadcast_to(np.asarray(a, np.float64), (nb,))
    base = model_oracle(oracle, model)
    raw = tag_size_ref.terms(base, arrays, tag_size)                 # uncorrected r, J
    T = tag_size_ref.terms(base, arrays, tag_size, kinds, a)
    w = np.array([float(loss_ref.rho(int(kinds[o]), float(a[o]), T.s[o])[1]) for o in range(nb)])
    # the entries that are exactly zero
    zero = np.zeros(T.n_params(), bool)
    zero[1:3] = not (model == RADIAL_FREE and not camera_const)
    if camera_const:
        zero[:3] = True
    seen_c, seen_t = np.zeros(nc, bool), np.zeros(nt, bool)
    seen_c[obs_cap] = True
    seen_t[obs_tag] = True
    cc = ~seen_c | (np.zeros(nc, bool) if cap_const is None else np.asarray(cap_const, bool))
    tc = ~seen_t | (np.zeros(nt, bool) if tag_const is None else np.asarray(tag_const, bool))
    zero[3:3 + 6 * nc] = np.repeat(cc, 6)
    zero[3 + 6 * nc:] = np.repeat(tc, 6)
    grad = np.where(zero, 0.0, T.grad)
    # tolerances, from the uncorrected rows
    r, J = raw.r, raw.J
    dr = RTOL * np.abs(r) + ATOL
    dJ = RTOL * np.max(np.abs(J), axis=2)                            # (nb, 8): the row's largest entry
    ds = np.sum(2.0 * np.abs(r) * dr, axis=1)
    r2 = np.array([rho2(int(kinds[o]), float(a[o]), T.s[o], ds[o]) for o in range(nb)])
    Jr = np.einsum("oij,oi->oj", J, r)
    dg_dr = np.abs(w[:, None, None] * J + 2.0 * r2[:, None, None] * r[:, :, None] * Jr[:, None, :])
    tol_o = np.einsum("oij,oi->oj", dg_dr, dr) + w[:, None] * np.sum(np.abs(r) * dJ, axis=1)[:, None]
    tol_g = np.zeros(T.n_params())
    tol_g[:3] = tol_o[:, :3].sum(0)
    np.add.at(tol_g[3:3 + 6 * nc].reshape(-1, 6), obs_cap, tol_o[:, 3:9])
    np.add.at(tol_g[3 + 6 * nc:].reshape(-1, 6), obs_tag, tol_o[:, 9:15])
    tol_g[zero] = 0.0
    return Reference(cost=T.cost, residuals=T.r, sq_norm=T.s, weight=w, gradient=grad, zero=zero,
                     tol_cost=0.5 * float(np.sum(w * ds)), tol_sq_norm=ds, tol_weight=np.abs(r2) * ds,
                     tol_gradient=tol_g)


def flat_gradient(g):
    """An evaluate() result's gradient dict as the flat vector."""
    return np.concatenate([g["camera"].ravel(), g["cap"].ravel(), g["tag"].ravel()])


def worst(got, ref):
    """name -> the largest |error| / tolerance of an evaluate() result against its Reference (an
    entry of zero tolerance counts as 0 when it is exact, inf otherwise)."""
    def ratio(err, tol):
        err, tol = np.abs(np.asarray(err, np.float64)).ravel(), np.asarray(tol, np.float64).ravel()
        if err.size == 0:
            return 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(tol > 0.0, err / np.where(tol > 0.0, tol, 1.0), np.where(err == 0.0, 0.0, np.inf))
        return float(np.max(q))
    out = {"cost": ratio(got["cost"] - ref.cost, ref.tol_cost),
           "sq_norm": ratio(got["sq_norm"] - ref.sq_norm, ref.tol_sq_norm),
           "weight": ratio(got["weight"] - ref.weight, np.maximum(ref.tol_weight, 0.0))}
    if got.get("residuals") is not None:
        out["residuals"] = ratio(got["residuals"] - ref.residuals, ref.tol_residuals())
    if got.get("gradient") is not None:
        out["gradient"] = ratio(flat_gradient(got["gradient"]) - ref.gradient, ref.tol_gradient)
    return out


def star(oracle, n=70, seed=11):
    """One tag seen by n captures and one capture seeing n tags, in one graph: captures 0..n-1 see
    tag 0, capture n sees tags 1..n.  Corners: the oracle's projection plus 0.5 px noise."""
    rng = np.random.default_rng(seed)
    camera = np.array([900.0, 0.0, 0.0])
    cap = np.zeros((n + 1, 6))
    cap[:n, :3] = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(1.2, 2.0, n)], 1)
    cap[:n, 3:] = rng.normal(0, 0.15, (n, 3))
    cap[n] = [0.0, 0.0, 2.5, 0.05, -0.03, 0.02]
    tag = np.zeros((n + 1, 6))
    tag[0, 3:] = [0.02, -0.04, 0.1]
    tag[1:, :3] = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.45, 0.45, n), rng.uniform(-0.1, 0.1, n)], 1)
    tag[1:, 3:] = rng.normal(0, 0.15, (n, 3))
    obs_cap = np.concatenate([np.arange(n), np.full(n, n)]).astype(np.int32)
    obs_tag = np.concatenate([np.zeros(n, int), 1 + np.arange(n)]).astype(np.int32)
    return project(oracle, (camera, cap, tag, obs_cap, obs_tag, np.zeros((2 * n, 8))), seed=seed)


def weights_separate(weight, bad):
    """(largest weight of the shifted observations, smallest of the others)."""
    mask = np.zeros(len(weight), bool)
    mask[bad] = True
    return float(np.max(weight[mask])), float(np.min(weight[~mask]))
