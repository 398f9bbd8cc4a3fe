"""The mapper (include/arslam_lm.h): the pointer-keyed ceres::Problem mirror and the bulk
struct-of-arrays path."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import (ALLREDUCE_FN, BLOCK_NONE, COMM_ID_BYTES, COV_OK, ITER_CB, SOLVER_ABORT, SOLVER_CONTINUE, CovInfo, CovPair,
                   EvaluateOptions, Iteration, Options, SoaProblem, StepInfo, Summary, _check, _dp, _f64, _load, _Owner,
                   _ptr, lib, make_options)


_NOT_ANCHORED = object()   # _covariance: the form is not an _anchored one (None is "anchored, no anchor")


class _Soa:
    def __init__(self, camera, cap, tag, obs_cap, obs_tag, corners, camera_const=False,
                 cap_const=None, tag_const=None):
        self.camera = _f64(camera).copy()
        self.cap = _f64(cap, (-1, 6)).copy()
        self.tag = _f64(tag, (-1, 6)).copy()
        self.obs_cap = np.ascontiguousarray(obs_cap, np.int32)
        self.obs_tag = np.ascontiguousarray(obs_tag, np.int32)
        self.corners = _f64(corners, (-1, 8))
        self.cap_const = None if cap_const is None else np.ascontiguousarray(cap_const, np.uint8)
        self.tag_const = None if tag_const is None else np.ascontiguousarray(tag_const, np.uint8)
        self.s = SoaProblem(self.cap.shape[0], self.tag.shape[0], self.obs_cap.shape[0],
                            _ptr(self.camera), _ptr(self.cap), _ptr(self.tag), _ptr(self.obs_cap),
                            _ptr(self.obs_tag), _ptr(self.corners), int(bool(camera_const)),
                            _ptr(self.cap_const), _ptr(self.tag_const))


def solve_soa(camera, cap, tag, obs_cap, obs_tag, corners, camera_const=False, cap_const=None,
              tag_const=None, loss=None, obs_loss=None, **opts):
    """One-shot bulk solve.  Returns (camera, cap, tag, summary dict).
    loss = (kind, a): every observation's robust loss; obs_loss = (kinds[n_obs], a[n_obs]): one per
    observation (see ResidentProblem)."""
    if loss is not None or obs_loss is not None:
        R = ResidentProblem(camera, cap, tag, obs_cap, obs_tag, corners, camera_const, cap_const, tag_const,
                            loss=loss, obs_loss=obs_loss, **opts)
        try:
            s = R.solve()
            return R.camera, R.cap, R.tag, s
        finally:
            R.close()
    A = _Soa(camera, cap, tag, obs_cap, obs_tag, corners, camera_const, cap_const, tag_const)
    s = Summary()
    _check(lib().arslam_lm_solve_soa(C.byref(A.s), C.byref(make_options(**opts)), C.byref(s)))
    return A.camera, A.cap, A.tag, s.to_dict()


def warm_up(device=0):
    """One small solve (the 'tiny' synthetic graph) on `device`: the process's one-time runtime
    start (the library's code objects loaded on first launch, its stream, page-locked buffers),
    which a first load would otherwise carry.  Returns its wall time (s)."""
    import time
    from .. import synth
    t = time.perf_counter()
    g = synth.config_graph("tiny")
    ResidentProblem(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, device=device).solve()
    return time.perf_counter() - t


def solve_graph(g, loss=None, obs_loss=None, **opts):
    return solve_soa(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners, loss=loss, obs_loss=obs_loss, **opts)


class _Handle(_Owner):
    _create, _destroy = "arslam_lm_create", "arslam_lm_destroy"

    def set_options(self, **opts):
        _check(lib().arslam_lm_set_options(self._h, C.byref(make_options(**opts))))

    def get_options(self) -> Options:
        o = Options()
        _check(lib().arslam_lm_get_options(self._h, C.byref(o)))
        return o

    def set_loss(self, kind, a=0.0):
        """The handle's default loss (LOSS_*, scale a): what add_residual_block gives the blocks
        added afterwards and a bulk load gives every observation.  Drops a loaded SoA problem."""
        _check(lib().arslam_lm_set_loss(self._h, int(kind), float(a)))

    def get_loss(self):
        """(kind, a) of the default loss."""
        k, a = C.c_int(0), C.c_double(0.0)
        _check(lib().arslam_lm_get_loss(self._h, C.byref(k), C.byref(a)))
        return k.value, a.value

    def set_tag_size(self, size):
        """The handle's default tag side in metres (DEFAULT_TAG_SIZE on creation): what
        add_residual_block gives the blocks added afterwards and a bulk load gives every tag.
        Drops a loaded SoA problem."""
        _check(lib().arslam_lm_set_tag_size(self._h, float(size)))

    def get_tag_size(self):
        s = C.c_double(0.0)
        _check(lib().arslam_lm_get_tag_size(self._h, C.byref(s)))
        return s.value

    def set_camera_model(self, model):
        """The handle's camera model, CAMERA_PINHOLE (on creation) or CAMERA_RADIAL: under RADIAL
        the camera block's l1, l2 are a known calibration the solve holds.  Drops a loaded problem
        and a kept covariance; the next load or solve uses it."""
        _check(lib().arslam_lm_set_camera_model(self._h, int(model)))

    def camera_model(self):
        m = C.c_int(0)
        _check(lib().arslam_lm_camera_model(self._h, C.byref(m)))
        return m.value

    def set_estimate_distortion(self, on=True):
        """Estimate the distortion (off on creation): under CAMERA_RADIAL, with the camera block not
        constant, l1 and l2 are parameters like f and camera[1], camera[2] come back estimated;
        ignored under CAMERA_PINHOLE.  Drops a loaded problem and a kept covariance.  While it is in
        effect several ranks, ELIM_MIXED on a set that mixes sides and the covariances whose camera
        output is one scalar are refused (UNSUPPORTED); ``covariance_lens`` and the other ``_lens``
        forms carry the camera block whole and work."""
        _check(lib().arslam_lm_set_estimate_distortion(self._h, int(on)))

    def estimate_distortion(self):
        v = C.c_int(0)
        _check(lib().arslam_lm_estimate_distortion(self._h, C.byref(v)))
        return bool(v.value)

    def set_iteration_callback(self, fn):
        """ceres::IterationCallback: fn(iteration dict) -> SOLVER_CONTINUE / SOLVER_ABORT /
        SOLVER_TERMINATE_SUCCESSFULLY (None = continue); fn=None removes it."""
        if fn is None:
            self._iter_cb = None
            _check(lib().arslam_lm_set_iteration_callback(self._h, C.cast(None, ITER_CB), None))
            return

        def tramp(ctx, it):
            try:
                d = {f: getattr(it.contents, f) for f, _ in Iteration._fields_}
                r = fn(d)
                return SOLVER_CONTINUE if r is None else int(r)
            except Exception:   # noqa: BLE001 -- a raising callback aborts the solve
                return SOLVER_ABORT
        self._iter_cb = ITER_CB(tramp)
        _check(lib().arslam_lm_set_iteration_callback(self._h, self._iter_cb, None))

    def debug_force_indefinite(self, step_mask):
        """Test hook: linear solves whose bit min(i,63) is set in step_mask see an indefinite
        reduced system (camera diagonal -1), i.e. an invalid LM step."""
        _check(lib().arslam_lm_debug_force_indefinite(self._h, step_mask & (2**64 - 1)))

    def debug_force_multirank(self, on=True):
        """Test hook: the multi-rank path (split, two-phase factorization, every collective) with
        one rank, so set_comm(0, 1, uid) makes a one-rank RCCL communicator on a one-GPU box."""
        _check(lib().arslam_lm_debug_force_multirank(self._h, 1 if on else 0))
        self._forced_multirank, self._sharded_ranks = bool(on), 1   # (the call resets the communicator)

    def debug_evaluate_times(self):
        """The last evaluate()'s device times under phase_timing=1, ms: {upload, k_eval_obs,
        k_eval_blocks, k_eval_tree, copy_back} (arslam_lm_debug_evaluate_times)."""
        ms = np.zeros(5)
        _check(lib().arslam_lm_debug_evaluate_times(self._h, _ptr(ms)))
        return dict(zip(("upload", "k_eval_obs", "k_eval_blocks", "k_eval_tree", "copy_back"), ms.tolist()))

    def debug_step_stages(self, radius, lin_exchange="packed"):
        """Every stage of one LM step of the loaded problem at its loaded point under `radius`
        (arslam_lm_debug_step_stages): a dict of the arslam_lm_step_info fields and
        ``g``, ``colnorm``, ``scale``, ``diag``, ``xc`` (n,) by the caller's slots; ``S``
        (n_reduced, n_reduced) the assembled system before the factorization, ``rhs``
        (n_reduced,) its right-hand side row, ``S_padded`` (n_padded, n_padded) every row of the
        padded system; ``row_slot`` (n_reduced,) the caller's slot of a row, -1 for padding; ``y``
        (n_reduced,) the reduced solution.

        On a sharded handle (made with ``comm=`` of several ranks, or ``force_multirank``) it is
        arslam_lm_debug_step_stages_sharded: a collective call, every rank with the same `radius`
        and `lin_exchange` ("packed": iteration 0's sums by the packed all-reduce; "ride": a second
        linearization's top sums in front of the top tiles).  ``S`` and ``rhs`` are then this
        rank's share, ``y`` is masked, and the dict also has ``held`` (n,) bool, ``row_class``
        (n_reduced,) 0 own / 1 top / 2 another rank's, and ``rank``, ``n_ranks``, ``n_top_tiles``,
        ``n_top_rows``, ``n_owned_captures``, ``n_active_ranks`` (see the header)."""
        info = StepInfo()
        L = lib()
        sharded = getattr(self, "_sharded_ranks", 1) > 1 or getattr(self, "_forced_multirank", False)
        shard = np.zeros(8, np.int32)
        ride = {"packed": 0, "ride": 1}[lin_exchange]

        def call(g, colnorm, scale, diag, held, S, slot, cls, y, xc):
            if sharded:
                return L.arslam_lm_debug_step_stages_sharded(self._h, float(radius), ride, C.byref(info), _ptr(shard),
                                                             g, colnorm, scale, diag, held, S, slot, cls, y, xc)
            return L.arslam_lm_debug_step_stages(self._h, float(radius), C.byref(info), g, colnorm, scale, diag, S, slot,
                                                 y, xc)
        _check(call(*[None] * 10))
        n, nR, N = info.n, info.n_reduced, info.n_padded
        v = {k: np.zeros(n) for k in ("g", "colnorm", "scale", "diag", "xc")}
        S = np.zeros((max(N, 1), max(N, 1)))
        slot = np.zeros(max(nR, 1), np.int32)
        cls = np.zeros(max(nR, 1), np.int32)
        held = np.zeros(max(n, 1), np.uint8)
        y = np.zeros(max(nR, 1))
        _check(call(_ptr(v["g"]), _ptr(v["colnorm"]), _ptr(v["scale"]), _ptr(v["diag"]), _ptr(held), _ptr(S), _ptr(slot),
                    _ptr(cls), _ptr(y), _ptr(v["xc"])))
        out = info.to_dict()
        out.update(v)
        S = S[:N, :N]
        out.update(S_padded=S, S=S[:nR, :nR].copy(), rhs=S[nR, :nR].copy() if N else np.zeros(0),
                   row_slot=slot[:nR], y=y[:nR])
        if sharded:
            out.update(held=held[:n].astype(bool), row_class=cls[:nR],
                       **dict(zip(("rank", "n_ranks", "n_top_tiles", "n_top_rows", "n_owned_captures",
                                   "n_active_ranks"), (int(s) for s in shard[:6]))), lin_exchange=lin_exchange)
        return out

    def set_comm(self, rank, nranks, uid):
        """Join the ranks' exchange: ``uid`` is an RCCL unique id (bytes, one GPU per
        rank) or a host all-reduce ``fn(array, op)`` reducing a numpy array in place
        (op "sum" or "max"), e.g. over torch.distributed gloo."""
        if callable(uid):
            fn = uid

            def tramp(ctx, buf, count, dtype, op):
                try:
                    ct = C.c_double if dtype == 0 else C.c_ubyte
                    arr = np.ctypeslib.as_array(C.cast(buf, C.POINTER(ct)), shape=(count,))
                    fn(arr, "sum" if op == 0 else "max")
                    return 0
                except Exception:   # noqa: BLE001 -- reported to the solver as a comm failure
                    return 1
            self._comm_cb = ALLREDUCE_FN(tramp)
            _check(lib().arslam_lm_set_comm_callback(self._h, rank, nranks, self._comm_cb, None))
        else:
            _check(lib().arslam_lm_set_comm(self._h, rank, nranks, uid))
        self._sharded_ranks = int(nranks)


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().arslam_comm_unique_id(buf))
    return buf.raw


def _evaluate(call, n_cap, n_tag, n_obs, apply_loss, residuals, gradient):
    """One arslam_lm_evaluate / _evaluate_blocks call (call(opt, cost, residuals, sq_norm, weight[,
    gradient])) into fresh arrays; the result dict of ResidentProblem.evaluate."""
    o = EvaluateOptions(1 if apply_loss else 0)
    cost = C.c_double(0.0)
    res = np.zeros((n_obs, 8)) if residuals else None
    sq = np.zeros(n_obs)
    w = np.zeros(n_obs)
    args = [C.byref(o), C.byref(cost), _ptr(res), _ptr(sq), _ptr(w)]
    out = {"cost": 0.0, "residuals": res, "sq_norm": sq, "weight": w, "gradient": None}
    if gradient is not None:
        g = np.zeros(3 + 6 * n_cap + 6 * n_tag) if gradient else None
        args.append(_ptr(g))
        if gradient:
            out["gradient"] = {"camera": g[:3], "cap": g[3:3 + 6 * n_cap].reshape(n_cap, 6),
                               "tag": g[3 + 6 * n_cap:].reshape(n_tag, 6)}
    _check(call(*args))
    out["cost"] = cost.value
    return out


class ResidentProblem(_Handle):
    """SoA problem uploaded once to HBM; ``solve()`` restarts from the loaded state."""

    def __init__(self, camera, cap, tag, obs_cap, obs_tag, corners, camera_const=False,
                 cap_const=None, tag_const=None, comm=None, force_multirank=False, loss=None, obs_loss=None,
                 tag_size=None, camera_model=None, estimate_distortion=None, **opts):
        """loss = (kind, a): the robust loss of every observation (the handle's default loss);
        obs_loss = (kinds[n_obs], a[n_obs]): one loss per observation, in observation order;
        tag_size = [n_tag] the tags' sides in metres (a scalar: every tag's); None: DEFAULT_TAG_SIZE;
        camera_model = CAMERA_PINHOLE / CAMERA_RADIAL (None: the handle's, PINHOLE);
        estimate_distortion = True: under CAMERA_RADIAL l1, l2 are estimated (set_estimate_distortion)."""
        super().__init__(**opts)
        if camera_model is not None:
            self.set_camera_model(camera_model)
        if estimate_distortion is not None:
            self.set_estimate_distortion(estimate_distortion)
        if force_multirank:
            self.debug_force_multirank(True)
        if comm is not None:
            self.set_comm(*comm)
        if loss is not None:
            self.set_loss(*loss)
        self.A = _Soa(camera, cap, tag, obs_cap, obs_tag, corners, camera_const, cap_const, tag_const)
        L = lib()
        _load(self._h, self.A.s, self.A.s.n_tag, self.A.s.n_obs, tag_size, obs_loss,
              L.arslam_lm_load_soa, L.arslam_lm_load_soa_loss, L.arslam_lm_load_soa_sized)

    def solve(self):
        s = Summary()
        _check(lib().arslam_lm_solve_loaded(self._h, C.byref(s)))
        return s.to_dict()

    def evaluate(self, apply_loss=True, residuals=True, gradient=True):
        """ceres::Problem::Evaluate at the values ``camera`` / ``cap`` / ``tag`` hold now (the results
        after a solve, the loaded values before one, anything written there): ``cost`` = 1/2 sum rho,
        ``residuals`` (n_obs, 8) corrected by sqrt(rho'), ``sq_norm`` (n_obs,) the uncorrected |r|^2,
        ``weight`` (n_obs,) rho' (1 without a loss; near 0 for a rejected detection) and ``gradient``
        {camera (3,), cap (n_cap, 6), tag (n_tag, 6)}, exactly 0 for constant and unseen blocks
        (arslam_lm_evaluate).  apply_loss=False: the plain r, 1/2 sum s and J'r.  residuals / gradient
        False: that output is not computed back (its key is None)."""
        n_cap, n_tag, n_obs = self.A.s.n_cap, self.A.s.n_tag, self.A.s.n_obs
        return _evaluate(lambda *a: lib().arslam_lm_evaluate(self._h, *a), n_cap, n_tag, n_obs, apply_loss, residuals,
                         gradient)

    def _covariance(self, lens, anchor=_NOT_ANCHORED):
        n_cap, n_tag = self.A.s.n_cap, self.A.s.n_tag
        cap = np.zeros((n_cap, 6, 6))
        tag = np.zeros((n_tag, 6, 6))
        cs = np.zeros(max(n_cap, 1), np.int32)
        ts = np.zeros(max(n_tag, 1), np.int32)
        info = CovInfo()
        out = {"cap": cap, "tag": tag, "cap_status": cs[:n_cap], "tag_status": ts[:n_tag]}
        if lens:
            cam = np.zeros((3, 3))
            cam_st = C.c_int(0)
            args = (_ptr(cap), _ptr(tag), _ptr(cam), _ptr(cs), _ptr(ts), C.byref(cam_st), C.byref(info))
            if anchor is _NOT_ANCHORED:
                _check(lib().arslam_lm_covariance_lens(self._h, *args))
            else:
                _check(lib().arslam_lm_covariance_anchored(self._h, *_anchor(anchor), *args))
            out.update(cam=cam, var_f=cam[0, 0] if cam_st.value == COV_OK else -1.0, cam_status=cam_st.value)
        else:
            var_f = C.c_double(0.0)
            _check(lib().arslam_lm_covariance(self._h, _ptr(cap), _ptr(tag), C.byref(var_f), _ptr(cs), _ptr(ts),
                                              C.byref(info)))
            out["var_f"] = var_f.value
        out["info"] = info.to_dict()
        return out

    def covariance(self):
        """Marginal covariances at the point the last ``solve()`` returned (arslam_lm_covariance):
        ``cap`` (n_cap, 6, 6), ``tag`` (n_tag, 6, 6), ``var_f``, ``cap_status`` / ``tag_status``
        (COV_*) and ``info`` (arslam_lm_cov_info as a dict).  Unit-variance residuals: times sigma^2."""
        return self._covariance(lens=False)

    def covariance_lens(self):
        """``covariance()`` with the camera block whole (arslam_lm_covariance_lens): ``cam`` (3, 3),
        the marginal of [f, l1, l2], and ``cam_status`` beside the other keys (``var_f`` = cam[0, 0]
        when the camera has a covariance, else -1).  Works under ``set_estimate_distortion``: l1, l2
        are then rows of H and every block is the marginal of that larger H.  Held l1, l2: their
        rows and columns of ``cam`` are 0 and the rest is ``covariance()``'s bits."""
        return self._covariance(lens=True)

    def _covariance_pairs(self, entry, pairs):
        flat = np.ascontiguousarray([[a[0], a[1], b[0], b[1]] for a, b in pairs], np.int32).reshape(-1, 4)
        n = len(flat)
        cov = np.zeros((n, 6, 6))
        st = np.zeros(max(n, 1), np.int32)
        info = CovInfo()
        _check(entry(self._h, _ptr(flat if n else None, C.POINTER(CovPair)), n, _ptr(cov if n else None), _ptr(st),
                     C.byref(info)))
        return cov, st[:n], info.to_dict()

    def covariance_pairs(self, pairs):
        """Cross-covariance blocks at the point the last ``solve()`` returned
        (arslam_lm_covariance_pairs).  pairs: a sequence of ((kind_a, index_a), (kind_b, index_b)),
        kind BLOCK_CAMERA (index 0), BLOCK_CAPTURE or BLOCK_TAG.  Returns ``cov`` (n, 6, 6): rows
        of a by columns of b (a pair with the camera: cov(f, pose) in the first six values, var(f)
        at [0, 0] for the camera against itself, 0 elsewhere), ``status`` (n,) (COV_*) and ``info``."""
        return self._covariance_pairs(lib().arslam_lm_covariance_pairs, pairs)

    def covariance_pairs_lens(self, pairs):
        """``covariance_pairs()`` over the matrix of ``covariance_lens()``
        (arslam_lm_covariance_pairs_lens): BLOCK_CAMERA is the 3-wide block [f, l1, l2] -- rows 0..2
        of the (6, 6) as a, columns 0..2 as b, the top-left (3, 3) against itself, 0 elsewhere."""
        return self._covariance_pairs(lib().arslam_lm_covariance_pairs_lens, pairs)

    def covariance_anchored(self, anchor):
        """``covariance_lens()`` in the gauge of ``anchor``: None, or (kind, index) of a capture or a
        tag (BLOCK_CAPTURE / BLOCK_TAG) held fixed for this call besides the constant blocks
        (arslam_lm_covariance_anchored) -- what the handle would return had that block been constant.
        The anchor's own status is COV_UNAVAILABLE.  Works under every e-block set, ELIM_MIXED
        included; the loaded problem and a later solve are untouched."""
        return self._covariance(lens=True, anchor=anchor)

    def covariance_pairs_anchored(self, anchor, pairs):
        """``covariance_pairs_lens()`` in the gauge of ``anchor`` (as ``covariance_anchored``;
        arslam_lm_covariance_pairs_anchored).  A pair that names the anchor is COV_UNAVAILABLE."""
        kind, index = _anchor(anchor)
        return self._covariance_pairs(lambda h, *a: lib().arslam_lm_covariance_pairs_anchored(h, kind, index, *a), pairs)

    def _camera_rows(self, call):
        cam = self.debug_reduced_rows()[2]
        n_cols = cam + 4
        rows = np.zeros((3, n_cols))
        slot = np.zeros(3, np.int32)
        _check(call(n_cols, _ptr(rows), _ptr(slot)))
        return rows, slot

    def debug_cov_camera_rows(self):
        """(rows (3, n_reduced + 1), row_slot (3,)): the camera's reduced rows f, l1, l2 of the
        covariance's reduced system at the point the last ``solve()`` returned -- no LM diagonal, the
        last column (the right-hand side) 0 (arslam_lm_debug_cov_camera_rows)."""
        return self._camera_rows(lambda *a: lib().arslam_lm_debug_cov_camera_rows(self._h, *a))

    def debug_reduced_rows(self):
        """(cap_row (n_cap,), tag_row (n_tag,), cam_row): the first reduced row of each block, -1 off
        the reduced side (arslam_lm_debug_reduced_rows)."""
        cr = np.zeros(max(self.A.s.n_cap, 1), np.int32)
        tr = np.zeros(max(self.A.s.n_tag, 1), np.int32)
        cam = C.c_int(-1)
        _check(lib().arslam_lm_debug_reduced_rows(self._h, _ptr(cr), _ptr(tr), C.byref(cam)))
        return cr[:self.A.s.n_cap], tr[:self.A.s.n_tag], cam.value

    def debug_camera_rows(self, radius):
        """(rows (3, n_reduced + 1), row_slot (3,)): the camera's reduced rows f, l1, l2 of the
        assembled reduced system at the loaded point under the given radius, the last column the
        rows' right-hand side entries (arslam_lm_debug_camera_rows)."""
        return self._camera_rows(lambda *a: lib().arslam_lm_debug_camera_rows(self._h, float(radius), *a))

    def owned_captures(self):
        """Indices of the captures this rank owns (every capture on one rank)."""
        n = C.c_int(0)
        _check(lib().arslam_lm_owned_captures(self._h, None, 0, C.byref(n)))
        out = (C.c_int * max(n.value, 1))()
        _check(lib().arslam_lm_owned_captures(self._h, out, n.value, C.byref(n)))
        return np.array(out[:n.value], np.int64)

    def debug_break_dependency(self, ticket):
        """Test hook: make one dependency wait of the factorization task graph unreachable."""
        out = C.c_long(-1)
        _check(lib().arslam_lm_debug_break_dependency(self._h, ticket, C.byref(out)))
        return out.value

    @property
    def camera(self):
        return self.A.camera

    @property
    def cap(self):
        return self.A.cap

    @property
    def tag(self):
        return self.A.tag


def _anchor(anchor):
    """(kind, index) of an anchored covariance form's anchor; None: (BLOCK_NONE, 0)."""
    if anchor is None:
        return BLOCK_NONE, 0
    kind, index = anchor
    return int(kind), int(index)


def _block(a, n=None):
    """The pointer of a parameter block: a float64 array of size n (C-contiguous), or with n None of
    size 3 or 6, as the covariance and gradient getters take it."""
    if n is None:
        if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.size in (3, 6)):
            raise TypeError("parameter block must be a float64 array of size 3 or 6")
    elif not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.size == n):
        raise TypeError(f"parameter block must be a C-contiguous float64 array of size {n}")
    return _ptr(a)


class Problem(_Handle):
    """ceres::Problem mirror with pointer-keyed parameter blocks (numpy arrays)."""

    def __init__(self, **opts):
        super().__init__(**opts)
        self._keep = []

    def add_residual_block(self, corners, camera, capture, tag, loss=None, size=None):
        """loss = (kind, a): this block's own robust loss; None: the handle's default (set_loss).
        size: the side of this block's tag in metres; None: the handle's default (set_tag_size)."""
        c = _f64(corners).reshape(8)
        self._keep += [camera, capture, tag]
        blocks = (self._h, _ptr(c), _block(camera, 3), _block(capture, 6), _block(tag, 6))
        if size is not None:
            kind, a = self.get_loss() if loss is None else loss
            _check(lib().arslam_lm_add_residual_block_sized(*blocks, float(size), int(kind), float(a)))
        elif loss is not None:
            _check(lib().arslam_lm_add_residual_block_loss(*blocks, int(loss[0]), float(loss[1])))
        else:
            _check(lib().arslam_lm_add_residual_block(*blocks))

    def set_parameter_block_constant(self, block):
        _check(lib().arslam_lm_set_parameter_block_constant(self._h, _ptr(block, _dp)))

    def set_parameter_block_variable(self, block):
        _check(lib().arslam_lm_set_parameter_block_variable(self._h, _ptr(block, _dp)))

    def num_residual_blocks(self):
        return lib().arslam_lm_num_residual_blocks(self._h)

    def solve(self):
        s = Summary()
        _check(lib().arslam_lm_solve(self._h, C.byref(s)))
        return s.to_dict()

    def evaluate(self, apply_loss=True, residuals=True):
        """ceres::Problem::Evaluate over the residual blocks in the order they were added, at the
        values the blocks hold now (arslam_lm_evaluate_blocks): ``cost``, ``residuals`` (n, 8),
        ``sq_norm`` (n,), ``weight`` (n,) as ResidentProblem.evaluate; the gradient is kept on the
        handle for ``gradient_block``."""
        n = self.num_residual_blocks()
        out = _evaluate(lambda *a: lib().arslam_lm_evaluate_blocks(self._h, *a), 0, 0, n, apply_loss, residuals, None)
        del out["gradient"]
        return out

    def gradient_block(self, block):
        """The block's (3,) or (6,) entries of the gradient of the last ``evaluate()``
        (arslam_lm_gradient_block); an LMError (STATE) when the problem changed since."""
        p = _block(block)
        out = np.zeros(block.size)
        _check(lib().arslam_lm_gradient_block(self._h, p, _ptr(out)))
        return out

    def _covariance_block(self, entry, *blocks):
        ptrs = [_block(b) for b in blocks]
        out = np.zeros((blocks[0].size, blocks[-1].size))
        st = C.c_int(0)
        _check(entry(self._h, *ptrs, _ptr(out), C.byref(st)))
        return out, st.value

    def covariance_block(self, block):
        """Covariance::GetCovarianceBlock(block, block) after ``solve()``: (6, 6) for a pose block,
        (3, 3) for the camera block (var(f) at [0, 0]); and its status (COV_*)."""
        return self._covariance_block(lib().arslam_lm_covariance_block, block)

    def covariance_block_pair(self, a, b):
        """Covariance::GetCovarianceBlock(a, b) after ``solve()`` in Ceres' shapes -- (6, 6), (3, 6),
        (6, 3) or (3, 3), the camera block 3 wide with cov(f, .) in its first row / column -- and its
        status (COV_*) (arslam_lm_covariance_block_pair)."""
        return self._covariance_block(lib().arslam_lm_covariance_block_pair, a, b)

    def covariance_block_lens(self, block):
        """``covariance_block`` with the camera's (3, 3) over [f, l1, l2] whole
        (arslam_lm_covariance_block_lens); works under ``set_estimate_distortion``."""
        return self._covariance_block(lib().arslam_lm_covariance_block_lens, block)

    def covariance_block_pair_lens(self, a, b):
        """``covariance_block_pair`` with the camera block's three rows / columns [f, l1, l2]
        (arslam_lm_covariance_block_pair_lens); works under ``set_estimate_distortion``."""
        return self._covariance_block(lib().arslam_lm_covariance_block_pair_lens, a, b)

    def covariance_block_anchored(self, anchor, block):
        """``covariance_block_lens`` in the gauge of ``anchor``, a pose block of the problem held fixed
        for the call, or None (arslam_lm_covariance_block_anchored): SetParameterBlockConstant(anchor)
        + Covariance::Compute without touching the problem.  Served from the kept result while the
        anchor stays the same.  Works under every e-block set, ELIM_MIXED included."""
        pa = None if anchor is None else _block(anchor, 6)
        return self._covariance_block(lambda h, *a: lib().arslam_lm_covariance_block_anchored(h, pa, *a), block)

    def covariance_block_pair_anchored(self, anchor, a, b):
        """``covariance_block_pair_lens`` in the gauge of ``anchor`` (arslam_lm_covariance_block_pair_anchored)."""
        pa = None if anchor is None else _block(anchor, 6)
        return self._covariance_block(lambda h, *x: lib().arslam_lm_covariance_block_pair_anchored(h, pa, *x), a, b)

    def reset(self):
        _check(lib().arslam_lm_reset(self._h))
        self._keep = []

    def debug_tag_pair_tile(self, tag_a, tag_b):
        """Where the loaded problem's reduced system couples tag blocks a and b: 2 an assembled
        tile, 1 a fill tile of the factor, 0 no tile, -1 not free tags (arslam_lm_debug.h)."""
        st = C.c_int(0)
        _check(lib().arslam_lm_debug_tag_pair_tile(self._h, _block(tag_a, 6), _block(tag_b, 6), C.byref(st)))
        return st.value
