"""numpy reference of the batched localizer with robust losses (test helper, no GPU).

One query is a single free 6-parameter block (the capture; tags and camera are
constant), so Ceres' trust-region loop reduces to 6x6 solves.  This restates
k_localize's control flow (csrc/localize.hip, itself a restatement of the
oracle's or_solve for one block) over oracle.residual_jacobian and
loss_ref.rho: per observation s = |r|^2 over its 8 residuals, rows scaled by
sqrt(rho'(s)), cost 1/2 sum rho(s), and J~'r~, J~'J~, the Jacobi scaling, the LM
diagonal, the model cost change, the step quality and every termination test on
the corrected quantities.  With every kind NONE it is the oracle's
localize_many (pinned in test_localize_loss.py).
"""
import sys

import numpy as np

import loss_ref

CONVERGENCE, NO_CONVERGENCE, FAILURE, SKIPPED = 0, 1, 2, -1
RULE_NONE, RULE_GRADIENT, RULE_PARAMETER, RULE_FUNCTION, RULE_MIN_RADIUS, RULE_MAX_ITERS, RULE_INVALID_STEPS, \
    RULE_EVAL_FAILED = 0, 1, 2, 3, 4, 5, 6, 7
DBL_MAX = sys.float_info.max

# the oracle's / the library's default options (Ceres 2.0 defaults, max_num_iterations = 50)
DEFAULTS = dict(max_num_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10,
                parameter_tolerance=1e-8, initial_trust_region_radius=1e4, max_trust_region_radius=1e16,
                min_trust_region_radius=1e-32, min_relative_decrease=1e-3, min_lm_diagonal=1e-6,
                max_lm_diagonal=1e32, max_num_consecutive_invalid_steps=5, jacobi_scaling=1)


def _loss_arrays(n_obs, kinds, scales):
    kinds = np.zeros(n_obs, np.int64) if kinds is None else np.broadcast_to(np.asarray(kinds), (n_obs,))
    scales = np.zeros(n_obs) if scales is None else np.broadcast_to(np.asarray(scales, np.float64), (n_obs,))
    return kinds, scales


class _Query:
    """The residual blocks of one query: evaluation at a pose x."""

    def __init__(self, oracle, camera, tags, corners, kinds, scales):
        self.oracle, self.camera, self.tags, self.corners = oracle, camera, tags, corners
        self.kinds, self.scales = kinds, scales

    def plain(self, x):
        """Uncorrected r (k, 8) and capture-block J (k, 8, 6)."""
        k = len(self.tags)
        r, J = np.zeros((k, 8)), np.zeros((k, 8, 6))
        for j in range(k):
            rj, Jj = self.oracle.residual_jacobian(self.camera, x, self.tags[j], self.corners[j])
            r[j], J[j] = rj, Jj[:, 3:9]
        return r, J

    def terms(self, x):
        """s (k,), rho (k,), rho' (k,) and the plain rows at x."""
        r, J = self.plain(x)
        s = np.einsum("ki,ki->k", r, r)
        rho, rho1 = np.zeros_like(s), np.zeros_like(s)
        for j in range(len(s)):
            p, p1 = loss_ref.rho(int(self.kinds[j]), float(self.scales[j]), s[j])
            rho[j], rho1[j] = float(p), float(p1)
        return s, rho, rho1, r, J

    def linearize(self, x):
        """(finite, cost, J~'r~ (6,), J~'J~ (6, 6))."""
        s, rho, rho1, r, J = self.terms(x)
        w = np.sqrt(rho1)
        rt, Jt = (w[:, None] * r).reshape(-1), (w[:, None, None] * J).reshape(-1, 6)
        return bool(np.isfinite(r).all()), 0.5 * float(rho.sum()), Jt.T @ rt, Jt.T @ Jt

    def cost(self, x):
        s, rho, _, r, _ = self.terms(x)
        return bool(np.isfinite(r).all()), 0.5 * float(rho.sum())


def solve_query(qr, x0, o):
    """The single-block LM from x0; returns a dict (status, rule, num_iterations, initial_cost,
    final_cost, pose)."""
    x = np.array(x0, np.float64)
    out = dict(status=SKIPPED, rule=RULE_NONE, num_iterations=0, num_successful_steps=0,
               num_unsuccessful_steps=0)
    finite, cost, g, H = qr.linearize(x)
    out["initial_cost"] = cost

    def done(status, rule):
        out.update(status=status, rule=rule, final_cost=cost, pose=x)
        return out

    if not finite:
        return done(FAILURE, RULE_EVAL_FAILED)
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H))) if o["jacobi_scaling"] else np.ones(6)
    radius, decrease = o["initial_trust_region_radius"], 2.0
    reuse_diag, succ, n_invalid, iteration = False, True, 0, 0
    x_norm = float(np.sqrt(x @ x))
    gmax = float(np.abs(g).max())
    diag = None
    while True:
        if succ:
            out["num_successful_steps"] += iteration > 0
        else:
            out["num_unsuccessful_steps"] += 1
        out["num_iterations"] += 1
        if iteration >= o["max_num_iterations"]:
            return done(NO_CONVERGENCE, RULE_MAX_ITERS)
        if succ and gmax <= o["gradient_tolerance"]:
            return done(CONVERGENCE, RULE_GRADIENT)
        if radius <= o["min_trust_region_radius"]:
            return done(CONVERGENCE, RULE_MIN_RADIUS)
        iteration += 1
        if not reuse_diag:
            diag = np.clip(scale * scale * np.diag(H), o["min_lm_diagonal"], o["max_lm_diagonal"])
        reuse_diag = True
        A = scale[:, None] * H * scale[None, :] + np.diag(diag / radius)
        valid, model, st = False, 0.0, None
        try:
            L = np.linalg.cholesky(A)
            y = np.linalg.solve(L.T, np.linalg.solve(L, scale * g))
            if np.isfinite(y).all():
                st = -scale * y
                model = -(float(g @ st) + 0.5 * float(st @ H @ st))
                valid = model > 0.0
        except np.linalg.LinAlgError:
            pass
        if not valid:
            n_invalid += 1
            if n_invalid >= o["max_num_consecutive_invalid_steps"]:
                return done(FAILURE, RULE_INVALID_STEPS)
            radius /= decrease
            decrease *= 2.0
            succ = False
            continue
        n_invalid = 0
        xc = x + st
        step_norm = float(np.sqrt((x - xc) @ (x - xc)))
        cfin, cand = qr.cost(xc)
        if not cfin:
            cand = DBL_MAX
        if step_norm <= o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]):
            return done(CONVERGENCE, RULE_PARAMETER)
        if abs(cost - cand) <= o["function_tolerance"] * cost:
            return done(CONVERGENCE, RULE_FUNCTION)
        quality = -DBL_MAX if cand >= DBL_MAX else (cost - cand) / model
        if quality > o["min_relative_decrease"]:
            x = xc
            x_norm = float(np.sqrt(x @ x))
            _, cost, g, H = qr.linearize(x)
            gmax = float(np.abs(g).max())
            succ = True
            t = 2.0 * quality - 1.0
            radius = min(radius / max(1.0 / 3.0, 1.0 - t * t * t), o["max_trust_region_radius"])
            decrease = 2.0
            reuse_diag = False
        else:
            succ = False
            radius /= decrease
            decrease *= 2.0


def _queries(oracle, batch, kinds, scales):
    kinds, scales = _loss_arrays(batch.obs_tag.shape[0], kinds, scales)
    camera = np.asarray(batch.camera, np.float64)
    tag = np.asarray(batch.tag, np.float64).reshape(-1, 6)
    corners = np.asarray(batch.corners, np.float64).reshape(-1, 8)
    for q in range(batch.n_query):
        a, b = int(batch.q_start[q]), int(batch.q_start[q + 1])
        yield q, a, b, _Query(oracle, camera, tag[batch.obs_tag[a:b]], corners[a:b], kinds[a:b], scales[a:b])


def observation_terms(oracle, batch, pose, kinds=None, scales=None, status=None):
    """Per observation the plain s = |r|^2 and w = rho'(s) at the given poses (n_query, 6);
    -1 for the observations of queries whose status is SKIPPED."""
    nb = batch.obs_tag.shape[0]
    s, w = np.full(nb, -1.0), np.full(nb, -1.0)
    for q, a, b, qr in _queries(oracle, batch, kinds, scales):
        if b == a or (status is not None and status[q] == SKIPPED):
            continue
        s[a:b], _, w[a:b], _, _ = qr.terms(np.asarray(pose[q], np.float64))
    return s, w


def localize(oracle, batch, kinds=None, scales=None, init_from_map=True, pose=None, **opts):
    """localizeMany with per-observation losses (kinds, scales: scalars, arrays [n_obs] or None).

    Returns a dict of arrays over the queries (status, rule, num_iterations, initial_cost,
    final_cost, pose (n_query, 6)) and over the observations (s, w at the returned pose; -1 for
    skipped queries)."""
    o = dict(DEFAULTS, **opts)
    nq = batch.n_query
    # the initial poses and the skip rule are the oracle's own (initCapturePose from the first
    # mapped block): zero iterations leave every query at its initial value
    pose0, status0, _ = oracle.localize_many(batch, init_from_map=init_from_map, pose=pose, max_num_iterations=0)
    out = dict(status=np.full(nq, SKIPPED), rule=np.zeros(nq, np.int64), num_iterations=np.zeros(nq, np.int64),
               initial_cost=np.zeros(nq), final_cost=np.zeros(nq), pose=np.array(pose0, np.float64))
    for q, a, b, qr in _queries(oracle, batch, kinds, scales):
        if status0[q] == SKIPPED:
            continue
        r = solve_query(qr, pose0[q], o)
        for key in ("status", "rule", "num_iterations", "initial_cost", "final_cost", "pose"):
            out[key][q] = r[key]
    out["s"], out["w"] = observation_terms(oracle, batch, out["pose"], kinds, scales, out["status"])
    return out


def shifted_batch(batch, seed=11, px=40.0):
    """A copy of `batch` with, in every query, one observation other than the first shifted by
    px pixels in a random direction (all four corners alike).  Returns (batch, shifted indices)."""
    import dataclasses
    rng = np.random.default_rng(seed)
    corners = np.array(batch.corners, np.float64).reshape(-1, 8).copy()
    bad = []
    for q in range(batch.n_query):
        a, b = int(batch.q_start[q]), int(batch.q_start[q + 1])
        if b - a < 2:
            continue
        o = a + 1 + int(rng.integers(0, b - a - 1))
        ang = rng.uniform(0, 2 * np.pi)
        corners[o] += np.tile([np.cos(ang) * px, np.sin(ang) * px], 4)
        bad.append(o)
    return dataclasses.replace(batch, corners=corners), np.array(bad, np.int64)
