"""The ArSlamSolver host mirror (include/arslam_slam.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import CovInfo, Summary, Transform, _check, _f64, _Owner, _ptr, lib


class SlamSolver(_Owner):
    """ArSlamSolver (ar_slam_util.hpp:361-497) over the C++ host mirror: captures, arucos and
    blocks addressed by index; uids / ids are strings."""
    _create, _destroy = "arslam_slam_create", "arslam_slam_destroy"

    def __init__(self, verbose=False, **opts):
        super().__init__(**opts)
        lib().arslam_slam_set_verbose(self._h, int(bool(verbose)))

    def set_loss(self, kind, a=0.0):
        """The robust loss (LOSS_*, scale a) of every residual block added from now on: solve,
        solve_incremental and the solveCapture calls inside them.  localize_many has its own:
        set_localize_loss."""
        _check(lib().arslam_slam_set_loss(self._h, int(kind), float(a)))

    def set_localize_loss(self, kind, a=0.0):
        """The robust loss (LOSS_*, scale a) of every residual block localize_many adds."""
        _check(lib().arslam_slam_set_localize_loss(self._h, int(kind), float(a)))

    def set_default_aruco_size(self, size):
        """The side (metres) of the tags created from now on (DEFAULT_TAG_SIZE initially)."""
        _check(lib().arslam_slam_set_default_aruco_size(self._h, float(size)))

    def set_aruco_size(self, tag_id, size):
        """The side (metres) of the tag with this id string; may precede its first detection.
        STATE once the tag is initialised or has residual blocks."""
        _check(lib().arslam_slam_set_aruco_size(self._h, str(tag_id).encode(), float(size)))

    def aruco_size(self, a):
        s = C.c_double(0.0)
        _check(lib().arslam_slam_aruco_size(self._h, int(a), C.byref(s)))
        return s.value

    def set_camera_model(self, model):
        """CAMERA_PINHOLE or CAMERA_RADIAL for the mapper and the localizer the solver keeps.
        STATE once residual blocks have been added."""
        _check(lib().arslam_slam_set_camera_model(self._h, int(model)))

    def camera_model(self):
        m = C.c_int(0)
        _check(lib().arslam_slam_camera_model(self._h, C.byref(m)))
        return m.value

    def camera_distortion(self):
        """The plumb_bob vector beside camera_info: [l1, l2, 0, 0, 0] under RADIAL, else zeros."""
        d = np.zeros(5)
        _check(lib().arslam_slam_camera_distortion(self._h, _ptr(d)))
        return d

    def load_yaml(self, path):
        _check(lib().arslam_slam_load_yaml(self._h, str(path).encode()))

    def load_yaml_string(self, text):
        _check(lib().arslam_slam_load_yaml_string(self._h, text.encode()))

    def save_yaml(self, path):
        _check(lib().arslam_slam_save_yaml(self._h, str(path).encode()))

    def add_detections(self, capture_uid, ids, corners, image_width=1020, image_height=768, image_path=""):
        """Detections.msg -> capture index, or None when ignored (addDetections :591-627)."""
        corners = _f64(corners, (-1, 8))
        n = corners.shape[0]
        if len(ids) != n:
            raise ValueError("one id per detection")
        arr = (C.c_char_p * max(n, 1))(*[str(i).encode() for i in ids])
        idx = C.c_int(-1)
        _check(lib().arslam_slam_add_detections(self._h, str(capture_uid).encode(), image_width, image_height,
                                                str(image_path).encode(), n, arr, _ptr(corners), C.byref(idx)))
        return None if idx.value < 0 else idx.value

    def solve(self):
        _check(lib().arslam_slam_solve(self._h))

    def solve_incremental(self):
        _check(lib().arslam_slam_solve_incremental(self._h))

    def localize_many(self, first_loc_cap_idx):
        _check(lib().arslam_slam_localize_many(self._h, first_loc_cap_idx))

    def localize_covariance(self, cap_idx):
        """(cov (6, 6), status COV_*) of a capture the last localize_many localized
        (Localizer.covariance); LMError -7 (STATE) for any other capture."""
        cov, st = np.zeros((6, 6)), C.c_int(-1)
        _check(lib().arslam_slam_localize_covariance(self._h, int(cap_idx), _ptr(cov), C.byref(st)))
        return cov, st.value

    def covariance(self, anchor):
        """The mapper problem's covariance in the gauge of aruco ``anchor`` (an index; it must have
        residual blocks in the problem), after solve() or solve_incremental()
        (arslam_slam_covariance and its getters): {cap (n, 6, 6), cap_status, aruco (n, 6, 6),
        aruco_status, cam (3, 3), cam_status, info}.  A capture or aruco that is not in the mapper
        problem (localized by localize_many, or not yet added) and the anchor itself are
        COV_UNAVAILABLE, -1 in their values."""
        info = CovInfo()
        _check(lib().arslam_slam_covariance(self._h, int(anchor), C.byref(info)))
        nc, na = self.num_captures, self.num_arucos
        cap, aruco, cam = np.zeros((nc, 6, 6)), np.zeros((na, 6, 6)), np.zeros((3, 3))
        cs, ast, st = np.zeros(nc, np.int32), np.zeros(na, np.int32), C.c_int(-1)
        for c in range(nc):
            _check(lib().arslam_slam_capture_covariance(self._h, c, _ptr(cap[c]), C.byref(st)))
            cs[c] = st.value
        for a in range(na):
            _check(lib().arslam_slam_aruco_covariance(self._h, a, _ptr(aruco[a]), C.byref(st)))
            ast[a] = st.value
        _check(lib().arslam_slam_camera_covariance(self._h, _ptr(cam), C.byref(st)))
        return {"cap": cap, "cap_status": cs, "aruco": aruco, "aruco_status": ast, "cam": cam, "cam_status": st.value,
                "info": info.to_dict()}

    def covariance_pair(self, anchor, a, b):
        """(cov (6, 6), status): block (a, b) of the same matrix, a and b (kind, index) with kind
        BLOCK_CAMERA (index 0), BLOCK_CAPTURE or BLOCK_TAG (an aruco); rows of a by columns of b,
        the camera three wide (arslam_slam_covariance_pair)."""
        cov, st = np.zeros((6, 6)), C.c_int(-1)
        _check(lib().arslam_slam_covariance_pair(self._h, int(anchor), int(a[0]), int(a[1]), int(b[0]), int(b[1]),
                                                 _ptr(cov), C.byref(st)))
        return cov, st.value

    def evaluate(self):
        """ceres::Problem::Evaluate on the mapper problem at the current poses
        (arslam_slam_evaluate): {cost, sq_norm (num_blocks,), weight (num_blocks,)}, the block's
        |r|^2 and loss weight rho' under the loss it was added with; -1 in both for a block that
        is not in the problem."""
        n = lib().arslam_slam_num_blocks(self._h)
        cost = C.c_double(0.0)
        sq, w = np.zeros(max(n, 1)), np.zeros(max(n, 1))
        _check(lib().arslam_slam_evaluate(self._h, C.byref(cost), _ptr(sq), _ptr(w)))
        return {"cost": cost.value, "sq_norm": sq[:n], "weight": w[:n]}

    @property
    def num_captures(self):
        return lib().arslam_slam_num_captures(self._h)

    @property
    def num_arucos(self):
        return lib().arslam_slam_num_arucos(self._h)

    @property
    def num_blocks(self):
        return lib().arslam_slam_num_blocks(self._h)

    @property
    def num_solves(self):
        return lib().arslam_slam_num_solves(self._h)

    def last_summary(self):
        s = Summary()
        _check(lib().arslam_slam_last_summary(self._h, C.byref(s)))
        return s.to_dict()

    def solve_summary(self, i):
        """Summary of optimize() call i."""
        s = Summary()
        _check(lib().arslam_slam_solve_summary(self._h, i, C.byref(s)))
        return s.to_dict()

    def solve_capture(self, i):
        """Index of the capture whose optimize() was call i (the drivers' visiting order)."""
        c = C.c_int(-1)
        _check(lib().arslam_slam_solve_capture(self._h, i, C.byref(c)))
        return c.value

    def solve_order(self):
        return [self.solve_capture(i) for i in range(self.num_solves)]

    def unsolved_captures(self):
        """The unsolved-capture set in its iteration order (begin() first)."""
        n = C.c_int(0)
        _check(lib().arslam_slam_unsolved_captures(self._h, None, 0, C.byref(n)))
        out = (C.c_int * max(n.value, 1))()
        _check(lib().arslam_slam_unsolved_captures(self._h, out, n.value, C.byref(n)))
        return [int(out[i]) for i in range(n.value)]

    def capture(self, c):
        buf = C.create_string_buffer(256)
        pose = np.zeros(6)
        _check(lib().arslam_slam_capture(self._h, c, buf, 256, _ptr(pose)))
        return buf.value.decode(), pose

    def set_capture_pose(self, c, pose):
        p = _f64(pose).reshape(6).copy()
        _check(lib().arslam_slam_set_capture_pose(self._h, c, _ptr(p)))

    def aruco(self, a):
        buf = C.create_string_buffer(256)
        pose = np.zeros(6)
        init = C.c_int(0)
        _check(lib().arslam_slam_aruco(self._h, a, buf, 256, _ptr(pose), C.byref(init)))
        return buf.value.decode(), pose, bool(init.value)

    def set_aruco_pose(self, a, pose):
        p = _f64(pose).reshape(6).copy()
        _check(lib().arslam_slam_set_aruco_pose(self._h, a, _ptr(p)))

    def block(self, b):
        c, a, added = C.c_int(), C.c_int(), C.c_int()
        rect = np.zeros(8)
        _check(lib().arslam_slam_block(self._h, b, C.byref(c), C.byref(a), _ptr(rect), C.byref(added)))
        return c.value, a.value, rect, bool(added.value)

    def camera(self):
        p = np.zeros(3)
        w, h = C.c_int(), C.c_int()
        _check(lib().arslam_slam_camera(self._h, _ptr(p), C.byref(w), C.byref(h)))
        return p, (None if w.value < 0 else (w.value, h.value))

    def set_camera(self, params):
        p = _f64(params).reshape(3).copy()
        _check(lib().arslam_slam_set_camera(self._h, _ptr(p)))

    def capture_poses(self):
        return np.array([self.capture(c)[1] for c in range(self.num_captures)]).reshape(-1, 6)

    def aruco_poses(self):
        return np.array([self.aruco(a)[1] for a in range(self.num_arucos)]).reshape(-1, 6)

    def get_transforms(self):
        n = C.c_int(0)
        _check(lib().arslam_slam_get_transforms(self._h, None, 0, C.byref(n)))
        arr = (Transform * max(n.value, 1))()
        _check(lib().arslam_slam_get_transforms(self._h, arr, n.value, C.byref(n)))
        return [(t.child_frame_id.decode(), np.array(t.translation[:]), np.array(t.rotation[:]))
                for t in arr[:n.value]]

    def camera_info(self):
        k, p = np.zeros(9), np.zeros(12)
        _check(lib().arslam_slam_camera_info(self._h, _ptr(k), _ptr(p)))
        return k.reshape(3, 3), p.reshape(3, 4)
