"""Component entry points (include/arslam_lm_debug.h): single kernels, host-only plans and probes,
for the tests and the tools."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import (ELIM_CAPTURES, OrderStep, PlanInfo, SoaProblem, SplitInfo, TilePlanFacts, _check, _f64, _ip, _ptr,
                   lib)
from .mapper import _Soa


def debug_slam_init_pose(which, rect, camera, pose_in, size=None):
    """The host mirror's initialisers alone (no device): which = "ar": initArPose from the capture's
    inv_pose, "capture": initCapturePose from the tag's pose; for a tag of side `size` (None: the
    call with the default argument).  arslam_slam_debug_init_pose."""
    rect, camera, pose_in = _f64(rect).reshape(8), _f64(camera).reshape(3), _f64(pose_in).reshape(6)
    out = np.zeros(6)
    _check(lib().arslam_slam_debug_init_pose({"ar": 0, "capture": 1}[which], _ptr(rect), _ptr(camera), _ptr(pose_in),
                                             0.0 if size is None else float(size), _ptr(out)))
    return out


def _residual_jacobian(entry, cam, cap, tag, corners, per_obs=(), lead=(), j_cols=15, rho=False):
    """The body of the five residual / Jacobian probes: entry(n, *lead, cam, cap, tag, corners,
    *per_obs, r, J[, rho]) over n independent observations, cam broadcast to (n, 3) and each
    (value, dtype) of per_obs to [n] (None stays NULL).  Returns (r (n, 8), J (n, 8, j_cols)[, rho (n,)])."""
    cap = _f64(cap, (-1, 6))
    n = cap.shape[0]
    cam = _f64(np.broadcast_to(np.asarray(cam, np.float64), (n, 3)))
    tag = _f64(tag, (-1, 6))
    corners = _f64(corners, (-1, 8))
    extra = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v), (n,)), dt)
             for v, dt in per_obs]
    out = (np.zeros((n, 8)), np.zeros((n, 8, j_cols))) + ((np.zeros(n),) if rho else ())
    _check(entry(n, *lead, *map(_ptr, (cam, cap, tag, corners, *extra, *out))))
    return out


def debug_residual_jacobian(cam, cap, tag, corners):
    """Device residuals (n,8) and Jacobians (n,8,15) of n independent observations."""
    return _residual_jacobian(lib().arslam_debug_residual_jacobian, cam, cap, tag, corners)


def debug_residual_jacobian_sized(cam, cap, tag, corners, size):
    """debug_residual_jacobian for tags of side size[n] (metres; a scalar: every tag's)."""
    return _residual_jacobian(lib().arslam_debug_residual_jacobian_sized, cam, cap, tag, corners,
                              [(size, np.float64)])


def debug_residual_jacobian_model(cam, cap, tag, corners, model, size=None):
    """debug_residual_jacobian under a camera model (CAMERA_*; cam rows = f, l1, l2), for tags of
    side size[n] (a scalar: every tag's; None: the default side)."""
    return _residual_jacobian(lib().arslam_debug_residual_jacobian_model, cam, cap, tag, corners,
                              [(size, np.float64)], lead=(int(model),))


def debug_residual_jacobian_distortion(cam, cap, tag, corners, size=None):
    """The radial model's residuals (n, 8) and the rows' two distortion columns (n, 8, 2),
    d r / d l1 and d r / d l2 (cam rows = f, l1, l2), for tags of side size[n] (None: default)."""
    return _residual_jacobian(lib().arslam_debug_residual_jacobian_distortion, cam, cap, tag, corners,
                              [(size, np.float64)], j_cols=2)


def debug_residual_jacobian_loss(cam, cap, tag, corners, kinds, a):
    """Device residuals (n,8) and Jacobians (n,8,15) of n independent observations after each one's
    robust loss (kinds[n] LOSS_*, a[n]): the rows times sqrt(rho'(s)); and rho(s) (n,)."""
    return _residual_jacobian(lib().arslam_debug_residual_jacobian_loss, cam, cap, tag, corners,
                              [(kinds, np.uint8), (a, np.float64)], rho=True)


def debug_angle_axis_rotate(w, p):
    """Device AngleAxisRotatePoint of n points: (out (n,3), branch (n,) 1 = Rodrigues, 0 = small angle)."""
    w = _f64(w, (-1, 3))
    p = _f64(p, (-1, 3))
    n = w.shape[0]
    out = np.zeros((n, 3))
    br = np.zeros(n, np.int32)
    _check(lib().arslam_debug_angle_axis_rotate(n, _ptr(w), _ptr(p), _ptr(out), _ptr(br)))
    return out, br


def debug_dense_llt(A, b, executor=0):
    """Device Cholesky + solve of the SPD matrix A (lower triangle used). Returns (L, y, info)."""
    A = _f64(A).copy()
    n = A.shape[0]
    b = _f64(b).reshape(n)
    y = np.zeros(n)
    info = C.c_int(0)
    _check(lib().arslam_debug_dense_llt_ex(n, _ptr(A), _ptr(b), _ptr(y), C.byref(info), executor))
    return A, y, info.value


def _u8_or_none(a, shape):
    return None if a is None else np.ascontiguousarray(np.asarray(a) != 0, np.uint8).reshape(shape)


def debug_tile_llt(A, b, tile_pattern=None, executor=0, col_class=None, fill_first=False):
    """Device Cholesky + solve of the SPD matrix A restricted to a lower tile pattern
    (arslam_debug_tile_llt): tile_pattern None (dense) or (T, T), T = (n + 1 + 63) // 64; col_class
    None or T values 0 / 1 (a two-phase plan on one rank); fill_first: the fill-first store over
    NaN fill tiles.  Returns (L (n, n), y, info, pattern (T, T) after fill, plan facts dict)."""
    A = _f64(A)
    n = A.shape[0]
    T = (n + 1 + 63) // 64
    b = _f64(b).reshape(n)
    pat = _u8_or_none(tile_pattern, (T, T))
    cls = _u8_or_none(col_class, (T,))
    Lf = np.zeros((n, n))
    y = np.zeros(n)
    out = np.zeros((T, T), np.uint8)
    info = C.c_int(0)
    facts = TilePlanFacts()
    _check(lib().arslam_debug_tile_llt(n, _ptr(A), _ptr(b), _ptr(pat), executor, _ptr(cls), 1 if fill_first else 0,
                                       _ptr(Lf), _ptr(y), _ptr(out), C.byref(info), C.byref(facts)))
    return Lf, y, info.value, out, facts.as_dict()


def debug_tile_plan(T, tile_pattern=None, col_class=None):
    """Host-only (no device): the plan debug_tile_llt builds for T tiles a side.  Returns (pattern
    (T, T) after fill, plan facts dict with dag_valid)."""
    pat = _u8_or_none(tile_pattern, (T, T))
    cls = _u8_or_none(col_class, (T,))
    out = np.zeros((T, T), np.uint8)
    facts = TilePlanFacts()
    _check(lib().arslam_debug_tile_plan(int(T), _ptr(pat), _ptr(cls), _ptr(out), C.byref(facts)))
    return out, facts.as_dict()


def _factor_pattern(tile_pattern, T):
    return None if tile_pattern is None else np.ascontiguousarray(tile_pattern, np.uint8).reshape(T, T)


def debug_selinv(A, tile_pattern=None):
    """Device selected inverse of the SPD matrix A on the tiles of its factor (the step behind
    ``covariance()``, alone).  tile_pattern: None for a dense matrix, else (T, T) with T =
    (n + 1 + 63) // 64, non-zero where lower tile (i, j) of A is taken.  Returns (Z (n, n): the
    inverse on the factor's tiles, 0 elsewhere; pattern (T, T): the factor's lower tile pattern; info)."""
    A = _f64(A)
    n = A.shape[0]
    T = (n + 1 + 63) // 64
    pat = _factor_pattern(tile_pattern, T)
    Z = np.zeros((n, n))
    out = np.zeros((T, T), np.uint8)
    info = C.c_int(0)
    _check(lib().arslam_debug_selinv(n, _ptr(A), _ptr(pat), _ptr(Z), _ptr(out), C.byref(info)))
    return Z, out, info.value


def debug_tile_solve(A, B, tile_pattern=None):
    """X = A^-1 B from the device's multi-right-hand-side tile solve alone (the step behind
    ``covariance_pairs()``): A (n, n) SPD, factored as ``debug_selinv`` factors it, B (n, nrhs).
    Returns (X (n, nrhs), info)."""
    A = _f64(A)
    n = A.shape[0]
    B = np.ascontiguousarray(B, np.float64).reshape(n, -1)
    pat = _factor_pattern(tile_pattern, (n + 1 + 63) // 64)
    X = np.zeros_like(B)
    info = C.c_int(0)
    _check(lib().arslam_debug_tile_solve(n, _ptr(A), _ptr(pat), B.shape[1], _ptr(B), _ptr(X), C.byref(info)))
    return X, info.value


def _soa_of(camera, cap, tag, obs_cap, obs_tag, corners=None, camera_const=False, cap_const=None, tag_const=None):
    """The problem of a host-only probe; corners None: zeros (the structure alone is read)."""
    if corners is None:
        corners = np.zeros((len(obs_cap), 8))
    return _Soa(camera, cap, tag, obs_cap, obs_tag, corners, camera_const, cap_const, tag_const)


def debug_reduced_plan(camera, cap, tag, obs_cap, obs_tag, corners, camera_const=False, cap_const=None,
                       tag_const=None, ordering=2, skip_zero_tiles=1):
    """Host-only symbolic analysis (no device): reduced layout + tile plan.  Returns (info dict, tag_row)."""
    A = _Soa(camera, cap, tag, obs_cap, obs_tag, corners, camera_const, cap_const, tag_const)
    info = PlanInfo()
    tag_row = np.zeros(max(A.tag.shape[0], 1), np.int32)
    _check(lib().arslam_debug_reduced_plan(C.byref(A.s), ordering, skip_zero_tiles, C.byref(info), _ptr(tag_row)))
    return info.to_dict(), tag_row[:A.tag.shape[0]]


def debug_reduced_plan_side(camera, cap, tag, obs_cap, obs_tag, corners=None, elimination=ELIM_CAPTURES):
    """Host-only: the reduced layout and tile plan of a fresh one-rank load under elimination
    (ELIM_CAPTURES, ELIM_TAGS or ELIM_MIXED).  Returns (side used, info dict)."""
    A = _soa_of(camera, cap, tag, obs_cap, obs_tag, corners)
    info = PlanInfo()
    side = lib().arslam_debug_reduced_plan_side(C.byref(A.s), elimination, C.byref(info))
    _check(min(side, 0))
    return side, info.to_dict()


def debug_order_memory(problems, elimination=ELIM_CAPTURES, ordering=2, forget_before=None):
    """Host-only: the problems in turn through one elimination-order memory, the first as a first
    one-rank load, each later one as a pointer-keyed reload that may keep the remembered order
    (forget_before[i]: drop the memory before problem i, as a reset does).  problems: dicts with
    camera, cap, tag, obs_cap, obs_tag and optionally corners, camera_const, cap_const, tag_const.
    Returns one dict per problem: side, order_reused, recomputed (a kept order replaced because its
    tile elimination tree grew too tall), etree_height, pad_rows, and tag_row / cap_row: the first
    reduced row of each original tag / capture, -1 for none."""
    soas = [_soa_of(q["camera"], q["cap"], q["tag"], q["obs_cap"], q["obs_tag"], q.get("corners"),
                    q.get("camera_const", False), q.get("cap_const"), q.get("tag_const")) for q in problems]
    n = len(soas)
    arr = (SoaProblem * n)(*[A.s for A in soas])
    steps = (OrderStep * n)()
    tag_rows = [np.zeros(max(A.tag.shape[0], 1), np.int32) for A in soas]
    cap_rows = [np.zeros(max(A.cap.shape[0], 1), np.int32) for A in soas]
    tr = (_ip * n)(*[_ptr(r) for r in tag_rows])
    cr = (_ip * n)(*[_ptr(r) for r in cap_rows])
    fb = None
    if forget_before is not None:
        fb = np.ascontiguousarray(forget_before, np.uint8)
        assert fb.shape == (n,)
    _check(lib().arslam_debug_order_memory(arr, n, int(elimination), int(ordering), _ptr(fb), steps, tr, cr))
    out = []
    for i, A in enumerate(soas):
        d = steps[i].to_dict()
        d["tag_row"] = tag_rows[i][:A.tag.shape[0]]
        d["cap_row"] = cap_rows[i][:A.cap.shape[0]]
        out.append(d)
    return out


def box_fingerprint(device=0):
    """The device's hand-off round trips (arslam_debug_box_fingerprint), a few ms of GPU time:
    the kind of MI355X box a measurement ran on."""
    out = (C.c_double * 6)()
    _check(lib().arslam_debug_box_fingerprint(int(device), out))
    return {"cas_poll_ns": out[0], "sc1_load_ns": out[1], "wt_store_ack_ns": out[2],
            "pingpong_ns": out[3], "pingpong_xcc": [int(out[4]), int(out[5])]}


def debug_dag_simulate(g, n_workers, seed=1, policy=0, started=None):
    """Host-only: one simulated interleaving of the persistent executor's protocol on g's one-rank
    plan (policy 0 random, 1-3 adversarial; + 16 without the in-flight cap on claimed targets;
    + 32 with round 5's cap, half the grid).  started=k: only k of the n_workers workgroups ever
    start.  True if every task finished, False on a deadlock."""
    A = _Soa(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    ok = C.c_int(-1)
    if started is None:
        _check(lib().arslam_debug_dag_simulate(C.byref(A.s), int(n_workers), seed, int(policy), C.byref(ok)))
    else:
        _check(lib().arslam_debug_dag_simulate_started(C.byref(A.s), int(n_workers), int(started), seed,
                                                       int(policy), C.byref(ok)))
    return bool(ok.value)


def debug_dag_workgroup_limit(k):
    """Process-wide test knob: later k_factor_dag launches let only their first k workgroups start
    (as if only k were resident); k <= 0 restores the whole grid."""
    _check(lib().arslam_debug_dag_workgroup_limit(int(k)))


def debug_dag_fault_detail(g, rec):
    """Host-only: the text an executor fault carries for fault record rec[8] (llt_plan.h
    DagFaultField) on g's one-rank plan."""
    A = _Soa(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    r = (C.c_int * 9)(*([int(v) for v in rec] + [0] * (9 - len(rec))))
    buf = C.create_string_buffer(4096)
    _check(lib().arslam_debug_dag_fault_detail(C.byref(A.s), r, buf, len(buf)))
    return buf.value.decode()


def debug_gather_extend(camera, cap, tag, obs_cap, obs_tag, corners, c0):
    """Host-only: the appended-problem Schur gather plan (the first c0 captures' plan extended by the
    rest) against a fresh plan of the whole problem.  Returns (identical, n_destinations)."""
    A = _Soa(camera, cap, tag, obs_cap, obs_tag, corners)
    same, nd = C.c_int(0), C.c_int(0)
    _check(lib().arslam_debug_gather_extend(C.byref(A.s), c0, C.byref(same), C.byref(nd)))
    return bool(same.value), nd.value


def debug_schur_store_table(nblk):
    """Host-only: k_schur's output-stage descriptors for captures of nblk distinct tags (1..10), in
    kernel order [tile (r, cc), cc <= r + 1][lane][register]: (offset, stored) -- the element's offset
    in the capture's block-packed slab and whether the lane stores it."""
    off = np.zeros((13, 64, 4), np.int32)
    stored = np.zeros((13, 64, 4), np.uint8)
    _check(lib().arslam_debug_schur_store_table(int(nblk), _ptr(off), _ptr(stored)))
    return off, stored


def debug_rank_split(camera, cap, tag, obs_cap, obs_tag, corners, nranks, rank):
    """Host-only: the multi-rank split the solver makes for `rank` of `nranks` (two-phase tile
    plan of that rank, its validity) and every capture's owner.  Returns (info dict, cap_owner)."""
    A = _Soa(camera, cap, tag, obs_cap, obs_tag, corners)
    info = SplitInfo()
    owner = np.zeros(max(A.cap.shape[0], 1), np.int32)
    _check(lib().arslam_debug_rank_split(C.byref(A.s), nranks, rank, C.byref(info), _ptr(owner)))
    return info.to_dict(), owner[:A.cap.shape[0]]


def debug_dag_tasks(g, nranks=1, rank=0):
    """Host-only: the factorization's task graph in the plan the solver makes for `rank` of `nranks`
    (1: the one-rank plan).  Returns {"tasks": [n, 4] (type, y, z, w; type 0 POTRF k = y, 1 TRSM,
    2 update item, 3 INV k = y) in ticket order, "phase": [n], "T", "phase_split", "n_phases",
    "root_inv_col": the column whose POTRF task also inverts L_kk and that has no INV task, or -1}."""
    A = _Soa(g.camera, g.cap, g.tag, g.obs_cap, g.obs_tag, g.corners)
    n, info = C.c_long(0), (C.c_int * 4)()
    _check(lib().arslam_debug_dag_tasks(C.byref(A.s), int(nranks), int(rank), None, None, 0, C.byref(n), info))
    tasks, phase = np.zeros((max(n.value, 1), 4), np.int32), np.zeros(max(n.value, 1), np.int32)
    _check(lib().arslam_debug_dag_tasks(C.byref(A.s), int(nranks), int(rank), _ptr(tasks), _ptr(phase), n.value,
                                        C.byref(n), info))
    return {"tasks": tasks[:n.value], "phase": phase[:n.value], "T": info[0], "phase_split": info[1],
            "n_phases": info[2], "root_inv_col": info[3]}


def debug_ceres_e_blocks(camera, cap, tag, obs_cap, obs_tag, corners=None, camera_const=False, cap_const=None,
                         tag_const=None):
    """Host-only: Ceres 2.0's DENSE_SCHUR e-block set (the rule ELIM_AUTO follows), as
    {captures, tags, camera, max_tag_obs}."""
    A = _soa_of(camera, cap, tag, obs_cap, obs_tag, corners, camera_const, cap_const, tag_const)
    out = np.zeros(4, np.int32)
    _check(lib().arslam_debug_ceres_e_blocks(C.byref(A.s), _ptr(out)))
    return dict(captures=int(out[0]), tags=int(out[1]), camera=int(out[2]), max_tag_obs=int(out[3]))


def debug_mixed_groups(camera, cap, tag, obs_cap, obs_tag, corners=None, camera_const=False, cap_const=None,
                       tag_const=None):
    """Host-only: Ceres' e-block set (e_cap, e_tag: 0/1 per capture / tag) and the ELIM_MIXED
    device problem's {groups, f_blocks, direct, max_blk}."""
    A = _soa_of(camera, cap, tag, obs_cap, obs_tag, corners, camera_const, cap_const, tag_const)
    out = np.zeros(4, np.int32)
    e_cap = np.zeros(max(A.cap.shape[0], 1), np.uint8)
    e_tag = np.zeros(max(A.tag.shape[0], 1), np.uint8)
    _check(lib().arslam_debug_mixed_groups(C.byref(A.s), _ptr(out), _ptr(e_cap), _ptr(e_tag)))
    return dict(groups=int(out[0]), f_blocks=int(out[1]), direct=int(out[2]), max_blk=int(out[3]),
                e_cap=e_cap[:A.cap.shape[0]], e_tag=e_tag[:A.tag.shape[0]])
