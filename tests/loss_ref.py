"""numpy reference of the robust losses (test helper, no GPU).

Ceres 2.0 semantics (loss_function.cc, corrector.cc): for one residual block
s = |r|^2 over its 8 residuals, the cost is 1/2 sum rho(s), and the
linearization uses r~ = sqrt(rho') r, J~ = sqrt(rho') J (every loss here has
rho'' <= 0, the corrector's alpha = 0 branch).  r and J come from
oracle.residual_jacobian, one call per observation; the oracle itself has no
loss.
"""
import dataclasses
import sys

import numpy as np

NONE, HUBER, SOFT_L_ONE, CAUCHY = 0, 1, 2, 3
DBL_MIN = sys.float_info.min


def rho(kind, a, s):
    """(rho(s), rho'(s)) of loss `kind` with scale a; s a float or an array."""
    s = np.asarray(s, np.float64)
    b = float(a) * float(a)
    if kind == NONE:
        return s.copy(), np.ones_like(s)
    if kind == HUBER:
        big = s > b
        rt = np.sqrt(np.where(big, s, 1.0))
        return np.where(big, 2.0 * a * rt - b, s), np.where(big, np.maximum(DBL_MIN, a / rt), 1.0)
    if kind == SOFT_L_ONE:
        tmp = np.sqrt(1.0 + s / b)
        return 2.0 * b * (tmp - 1.0), np.maximum(DBL_MIN, 1.0 / tmp)
    if kind == CAUCHY:
        sm = 1.0 + s / b
        return b * np.log(sm), np.maximum(DBL_MIN, 1.0 / sm)
    raise ValueError(f"unknown loss kind {kind}")


def outliers(g):
    """g with 5 % of its observations shifted by 40 px in a random direction (all four corners of
    the observation alike).  Returns (graph, indices of the shifted observations)."""
    nb = g.n_obs
    rng = np.random.default_rng(5)
    bad = rng.choice(nb, int(0.05 * nb), replace=False)
    ang = rng.uniform(0, 2 * np.pi, len(bad))
    corners = np.array(g.corners, np.float64).reshape(nb, 8).copy()
    corners[bad] += np.tile(np.stack([np.cos(ang), np.sin(ang)], 1) * 40.0, (1, 4))
    return dataclasses.replace(g, corners=corners), bad


def _arrays(g_or_arrays):
    if isinstance(g_or_arrays, (tuple, list)):
        camera, cap, tag, obs_cap, obs_tag, corners = g_or_arrays
    else:
        g = g_or_arrays
        camera, cap, tag, obs_cap, obs_tag, corners = g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners
    return (np.asarray(camera, np.float64), np.asarray(cap, np.float64).reshape(-1, 6),
            np.asarray(tag, np.float64).reshape(-1, 6), np.asarray(obs_cap), np.asarray(obs_tag),
            np.asarray(corners, np.float64).reshape(-1, 8))


class RobustTerms:
    """cost = 1/2 sum rho; r (nb, 8) and J (nb, 8, 15: camera 3 | capture 6 | tag 6) corrected;
    rho (nb,); s (nb,) the uncorrected |r|^2; grad = J~' r~ over the parameter vector
    [camera 3 | captures 6 nc | tags 6 nt]."""

    def __init__(self, oracle, g_or_arrays, kinds, a):
        camera, cap, tag, obs_cap, obs_tag, corners = _arrays(g_or_arrays)
        nb = len(obs_cap)
        self.nc, self.nt, self.obs_cap, self.obs_tag = len(cap), len(tag), obs_cap, obs_tag
        kinds = np.broadcast_to(np.asarray(kinds), (nb,))
        a = np.broadcast_to(np.asarray(a, np.float64), (nb,))
        self.r = np.zeros((nb, 8))
        self.J = np.zeros((nb, 8, 15))
        self.s = np.zeros(nb)
        self.rho = np.zeros(nb)
        for o in range(nb):
            r, J = oracle.residual_jacobian(camera, cap[obs_cap[o]], tag[obs_tag[o]], corners[o])
            self.s[o] = float(r @ r)
            p, p1 = rho(int(kinds[o]), float(a[o]), self.s[o])
            w = np.sqrt(p1)
            self.rho[o] = p
            self.r[o] = w * r
            self.J[o] = w * J
        self.cost = 0.5 * float(np.sum(self.rho))
        self.grad = self.jt_times(self.r)

    def n_params(self):
        return 3 + 6 * self.nc + 6 * self.nt

    def jt_times(self, v):
        """J~' v for v (nb, 8)."""
        out = np.zeros(self.n_params())
        JTv = np.einsum("oij,oi->oj", self.J, v)
        out[:3] = JTv[:, :3].sum(0)
        np.add.at(out[3:3 + 6 * self.nc].reshape(-1, 6), self.obs_cap, JTv[:, 3:9])
        np.add.at(out[3 + 6 * self.nc:].reshape(-1, 6), self.obs_tag, JTv[:, 9:15])
        return out

    def j_times(self, delta):
        """J~ delta (nb, 8) for delta over the parameter vector."""
        d = np.concatenate([np.broadcast_to(delta[:3], (len(self.obs_cap), 3)),
                            delta[3:3 + 6 * self.nc].reshape(-1, 6)[self.obs_cap],
                            delta[3 + 6 * self.nc:].reshape(-1, 6)[self.obs_tag]], 1)
        return np.einsum("oij,oj->oi", self.J, d)

    def dense_jacobian(self):
        """J~ as one (8 nb, n_params) matrix (small graphs)."""
        nb = len(self.obs_cap)
        D = np.zeros((8 * nb, self.n_params()))
        for o in range(nb):
            rows = slice(8 * o, 8 * o + 8)
            D[rows, :3] = self.J[o][:, :3]
            c0, t0 = 3 + 6 * self.obs_cap[o], 3 + 6 * self.nc + 6 * self.obs_tag[o]
            D[rows, c0:c0 + 6] = self.J[o][:, 3:9]
            D[rows, t0:t0 + 6] = self.J[o][:, 9:15]
        return D

    def model_cost_change(self, delta):
        """Ceres' model cost change of the step delta: -(J~ d) . (r~ + J~ d / 2)."""
        jd = self.j_times(delta)
        return -float(np.sum(jd * (self.r + 0.5 * jd)))


def robust_terms(oracle, g_or_arrays, kinds, a):
    """The robust cost, corrected rows and gradient of a graph (or a (camera, cap, tag, obs_cap,
    obs_tag, corners) tuple) under per-observation losses (kinds, a: scalars or arrays)."""
    return RobustTerms(oracle, g_or_arrays, kinds, a)


def pack(camera, cap, tag):
    return np.concatenate([np.asarray(camera, np.float64).ravel(), np.asarray(cap, np.float64).ravel(),
                           np.asarray(tag, np.float64).ravel()])
