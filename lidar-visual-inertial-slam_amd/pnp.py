"""Python handle over include/lvi_pnp.h: KeyFrame::PnPRANSAC's cv::solvePnPRansac(matched_3d, matched_2d_old_norm, K = I,
D, rvec, t, true, 100, 10.0 / 460.0, 0.99, inliers) (keyframe.cpp:135-176) on the GPU, reduced to the inlier status
findConnection reads — a restatement of OpenCV 4.5.x, DESIGN §16.

A separate ABI from include/lvi_hotpath.h: only the product library exports it, so its signature table lives here and
is bound against ``liblvi_hip.so`` alone."""
import ctypes as C

import numpy as np

from . import _abi as A

_P = C.POINTER
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double

PATH_DIRECT, PATH_RANSAC = 1, 2
PATH_NAMES = {PATH_DIRECT: "direct", PATH_RANSAC: "ransac"}
MAX_POINTS, MAX_ITERS = 2048, 1024
# keyframe.cpp:163: the double 10.0 / 460.0 arrives in solvePnPRansac's `float reprojectionError`
REPROJECTION_ERROR = float(np.float32(10.0 / 460.0))


class PnPInfo(C.Structure):
    _fields_ = [("path", C.c_int32), ("iters", C.c_int32), ("n_subsets", C.c_int32), ("best_iter", C.c_int32), ("n_inliers", C.c_int32),
                ("which_beta", C.c_int32), ("R", C.c_double * 9), ("t", C.c_double * 3), ("stream_us", C.c_double)]


# name -> (restype, argtypes), one entry per function of include/lvi_pnp.h
PNP_SIGNATURES = {
    "lvi_pnp_abi_version": (_i32, []),
    "lvi_pnp_create": (_i32, [_i32, _i32, _i32, _P(_vp)]),
    "lvi_pnp_destroy": (None, [_vp]),
    "lvi_pnp_solve": (_i32, [_vp, _vp, _vp, _i32, _f64, _f64, _vp, _P(PnPInfo)]),
    "lvi_pnp_trace": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _P(_i32)]),
}


def bind(lib):
    """set the pnp signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(PNP_SIGNATURES)


def _info_dict(info):
    return dict(path=PATH_NAMES.get(info.path, info.path), iters=info.iters, n_subsets=info.n_subsets, best_iter=info.best_iter,
                n_inliers=info.n_inliers, which_beta=info.which_beta, R=np.array(info.R[:], np.float64).reshape(3, 3),
                t=np.array(info.t[:], np.float64), stream_us=info.stream_us)


class PnPRansac(A.Owned):
    """the inlier status of cv::solvePnPRansac(pts3d, pts2d, I, [], ..., max_iters, threshold, confidence, inliers) on the
    GPU.  One handle serves calls of up to max_points correspondences."""
    _destroy = "lvi_pnp_destroy"

    def __init__(self, lib, device=0, max_points=MAX_POINTS, max_iters=100):
        self.lib = bind(lib)
        self.max_points = int(max_points)
        self.max_iters = int(max_iters)
        self._h = C.c_void_p()
        lib.check(lib.dll.lvi_pnp_create(int(device), self.max_points, self.max_iters, C.byref(self._h)), "lvi_pnp_create")

    def solve(self, pts3d, pts2d, threshold=REPROJECTION_ERROR, confidence=0.99, with_info=False):
        """pts3d [n, 3], pts2d [n, 2] (f32) -> status [n] uint8 (and the info dict)"""
        a = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(pts2d, np.float32).reshape(-1, 2)
        if len(a) != len(b):
            raise ValueError("pts3d and pts2d differ in length")
        st = np.zeros(max(len(a), 1), np.uint8)
        info = PnPInfo()
        self.lib.check(self.lib.dll.lvi_pnp_solve(self._h, A._ptr(a), A._ptr(b), len(a), float(threshold), float(confidence), A._ptr(st),
                                                  C.byref(info)), "lvi_pnp_solve")
        st = st[:len(a)].copy()
        return (st, _info_dict(info)) if with_info else st

    def trace(self):
        """the last solve's hypotheses: subsets [m, 5], has_model [m], R [m, 3, 3], t [m, 3], good [m]"""
        m = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_pnp_trace(self._h, None, None, None, None, 0, C.byref(m)), "lvi_pnp_trace")
        k = max(m.value, 1)
        sub = np.zeros((k, 5), np.int32); has = np.zeros(k, np.int32); Rt = np.zeros((k, 12), np.float64); good = np.zeros(k, np.int32)
        self.lib.check(self.lib.dll.lvi_pnp_trace(self._h, A._ptr(sub), A._ptr(has), A._ptr(Rt), A._ptr(good), m.value, C.byref(m)), "lvi_pnp_trace")
        n = m.value
        return dict(subsets=sub[:n].copy(), has_model=has[:n].copy(), R=Rt[:n, :9].reshape(-1, 3, 3).copy(), t=Rt[:n, 9:].copy(), good=good[:n].copy())
