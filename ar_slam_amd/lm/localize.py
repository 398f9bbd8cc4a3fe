"""The batched localizer (include/arslam_localize.h): one-shot and resident."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import (LOSS_NONE, RULES, LocalizeBatchC, LocalizeResult, _check, _f64, _load, _Owner, _per, _ptr, lib,
                   make_options)


def _loc_results(res):
    n = len(res)
    f = {k: np.array([getattr(r, k) for r in res]) for k, _ in LocalizeResult._fields_}
    f["rule_name"] = [RULES.get(r, str(r)) for r in f["rule"]] if n else []
    return f


class _LocArrays:
    def __init__(self, batch, init_from_map, pose):
        self.camera = _f64(batch.camera).copy()
        self.tag = _f64(batch.tag, (-1, 6)).copy()
        self.q_start = np.ascontiguousarray(batch.q_start, np.int32)
        self.obs_tag = np.ascontiguousarray(batch.obs_tag, np.int32)
        self.corners = _f64(batch.corners, (-1, 8))
        nq = self.q_start.shape[0] - 1
        self.pose = np.zeros((nq, 6)) if pose is None else _f64(pose, (-1, 6)).copy()
        tim = getattr(batch, "tag_in_map", None)
        self.tim = None if tim is None else np.ascontiguousarray(tim, np.uint8)
        self.s = LocalizeBatchC(nq, self.tag.shape[0], self.obs_tag.shape[0],
                                _ptr(self.camera), _ptr(self.tag), _ptr(self.tim), _ptr(self.q_start),
                                _ptr(self.obs_tag), _ptr(self.corners), _ptr(self.pose), int(bool(init_from_map)))


def localize_many(batch, init_from_map=True, pose=None, loss=None, covariance=False, tag_size=None, **opts):
    """localizeMany on the device (one-shot).  ``batch`` has camera, tag, q_start, obs_tag,
    corners, tag_in_map (synth.LocalizeBatch).  loss = (kind, a): every observation's robust loss
    (LOSS_*, scale); the results' costs are then the robust cost.  tag_size: the map tags' sides in
    metres, [n_tag] or a scalar (None: DEFAULT_TAG_SIZE).  Returns (pose (Nq,6), results
    dict of arrays); with covariance=True also cov (Nq, 6, 6) and its status (Nq,), COV_*
    (Localizer.covariance)."""
    A = _LocArrays(batch, init_from_map, pose)
    nq = A.s.n_query
    res = (LocalizeResult * max(nq, 1))()
    cov = st = None
    if covariance:
        cov, st = np.zeros((max(nq, 1), 6, 6)), np.zeros(max(nq, 1), np.int32)
    kind, a = (LOSS_NONE, 0.0) if loss is None else (int(loss[0]), float(loss[1]))
    batch_opts = (C.byref(A.s), C.byref(make_options(**opts)))
    if tag_size is not None:
        _check(lib().arslam_localize_many_sized(*batch_opts, _ptr(_per(tag_size, A.s.n_tag)), kind, a, res,
                                                _ptr(cov), _ptr(st)))
    elif covariance:
        _check(lib().arslam_localize_many_cov(*batch_opts, kind, a, res, _ptr(cov), _ptr(st)))
    elif loss is None:
        _check(lib().arslam_localize_many(*batch_opts, res))
    else:
        _check(lib().arslam_localize_many_loss(*batch_opts, kind, a, res))
    out = (A.pose, _loc_results(res[:nq]))
    return out + (cov[:nq], st[:nq]) if covariance else out


class Localizer(_Owner):
    """Resident batched localizer: load a batch once, solve it many times."""
    _create, _destroy = "arslam_localizer_create", "arslam_localizer_destroy"

    def __init__(self, batch, init_from_map=True, pose=None, loss=None, obs_loss=None, tag_size=None,
                 camera_model=None, **opts):
        """loss = (kind, a): the robust loss of every observation (the handle's default loss);
        obs_loss = (kinds[n_obs], a[n_obs]): one loss per observation of this batch, in observation
        order, overriding the default; tag_size: the map tags' sides in metres, [n_tag] or a scalar
        (None: DEFAULT_TAG_SIZE); camera_model = CAMERA_PINHOLE / CAMERA_RADIAL (None: PINHOLE)."""
        super().__init__(**opts)
        if camera_model is not None:
            self.set_camera_model(camera_model)
        self.A = _LocArrays(batch, init_from_map, pose)
        self.n_query = self.A.s.n_query
        self.n_obs = self.A.s.n_obs
        if loss is not None:
            self.set_loss(*loss)
        L = lib()
        _load(self._h, self.A.s, self.A.s.n_tag, self.n_obs, tag_size, obs_loss,
              L.arslam_localizer_load, L.arslam_localizer_load_loss, L.arslam_localizer_load_sized)

    def set_camera_model(self, model):
        """CAMERA_PINHOLE or CAMERA_RADIAL (l1, l2 = the batch's camera[1], camera[2]): the model
        of solve(), observation_terms() and covariance(); the batch stays loaded."""
        _check(lib().arslam_localizer_set_camera_model(self._h, int(model)))

    def camera_model(self):
        m = C.c_int(0)
        _check(lib().arslam_localizer_camera_model(self._h, C.byref(m)))
        return m.value

    def set_tag_size(self, size):
        """The default side (metres) of every map tag of a batch loaded afterwards."""
        _check(lib().arslam_localizer_set_tag_size(self._h, float(size)))

    def get_tag_size(self):
        s = C.c_double(0.0)
        _check(lib().arslam_localizer_get_tag_size(self._h, C.byref(s)))
        return s.value

    def set_loss(self, kind, a=0.0):
        """The default loss (LOSS_*, scale a) of every observation, from the next solve() on; the
        loaded batch stays loaded.  A batch loaded with obs_loss keeps its own losses."""
        _check(lib().arslam_localizer_set_loss(self._h, int(kind), float(a)))

    def get_loss(self):
        """(kind, a) of the default loss."""
        k, a = C.c_int(0), C.c_double(0.0)
        _check(lib().arslam_localizer_get_loss(self._h, C.byref(k), C.byref(a)))
        return k.value, a.value

    def observation_terms(self):
        """(s, w), each (n_obs,): per observation the plain squared residual s = |r|^2 and the
        weight w = rho'(s) at the poses the last solve() returned (w = 1 without a loss, near 0 for
        a rejected detection); -1 for the observations of skipped queries."""
        s, w = np.zeros(max(self.n_obs, 1)), np.zeros(max(self.n_obs, 1))
        _check(lib().arslam_localizer_observation_terms(self._h, _ptr(s), _ptr(w)))
        return s[:self.n_obs], w[:self.n_obs]

    def covariance(self, timed=False):
        """(cov (n_query, 6, 6), status (n_query,), min_pivot (n_query,)): per query the inverse
        of J~'J~ at the pose the last solve() returned, rows corrected by the loss as in the solve
        (ceres::Covariance with apply_loss_function), parameters [t_c, w_c], for unit-variance
        residuals (multiply by the pixel noise's sigma^2); status COV_OK, COV_UNAVAILABLE (skipped
        or failed evaluation) or COV_RANK_DEFICIENT, the last two with cov = -1; min_pivot the
        smallest squared pivot of the equilibrated Cholesky.  timed=True appends the kernel's
        device time in ms."""
        nq = self.n_query
        cov, st, mp = np.zeros((max(nq, 1), 6, 6)), np.zeros(max(nq, 1), np.int32), np.zeros(max(nq, 1))
        ms = C.c_double(0.0)
        args = (self._h, _ptr(cov), _ptr(st), _ptr(mp))
        if timed:
            _check(lib().arslam_localizer_covariance_timed(*args, C.byref(ms)))
            return cov[:nq], st[:nq], mp[:nq], ms.value
        _check(lib().arslam_localizer_covariance(*args))
        return cov[:nq], st[:nq], mp[:nq]

    def solve(self, download=True):
        """Returns (pose or None, results or None, kernel_ms)."""
        ms = C.c_double(0.0)
        pose = np.zeros((self.n_query, 6)) if download else None
        res = (LocalizeResult * max(self.n_query, 1))() if download else None
        _check(lib().arslam_localizer_solve(self._h, _ptr(pose), res, C.byref(ms)))
        return pose, (None if res is None else _loc_results(res[:self.n_query])), ms.value
