"""Python handle over include/lvi_fmat.h: rejectWithF's cv::findFundamentalMat(un_cur, un_forw, FM_RANSAC, F_THRESHOLD,
0.99, status) (feature_tracker.cpp:209-242) on the GPU — a restatement of OpenCV 4.5.x, DESIGN §11.

A separate ABI from include/lvi_hotpath.h: only the product library exports it, so its signature table lives here and
is bound against ``liblvi_hip.so`` alone."""
import ctypes as C

import numpy as np

from . import _abi as A

_P = C.POINTER
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double

PATH_KERNEL, PATH_LMEDS, PATH_RANSAC = 1, 2, 3
PATH_NAMES = {PATH_KERNEL: "kernel", PATH_LMEDS: "lmeds", PATH_RANSAC: "ransac"}


class FmatInfo(C.Structure):
    _fields_ = [("path", C.c_int32), ("iters", C.c_int32), ("n_subsets", C.c_int32), ("best_iter", C.c_int32), ("best_root", C.c_int32),
                ("n_inliers", C.c_int32), ("best_median", C.c_double), ("F", C.c_double * 9), ("stream_us", C.c_double)]


# name -> (restype, argtypes), one entry per function of include/lvi_fmat.h
FMAT_SIGNATURES = {
    "lvi_fmat_abi_version": (_i32, []),
    "lvi_fmat_create": (_i32, [_i32, _i32, _i32, _P(_vp)]),
    "lvi_fmat_destroy": (None, [_vp]),
    "lvi_fmat_set_check_subset": (_i32, [_vp, _i32]),
    "lvi_fmat_find": (_i32, [_vp, _vp, _vp, _i32, _f64, _f64, _vp, _P(FmatInfo)]),
    "lvi_fmat_trace": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _P(_i32)]),
}


def bind(lib):
    """set the fmat signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(FMAT_SIGNATURES)


def _info_dict(info):
    return dict(path=PATH_NAMES.get(info.path, info.path), iters=info.iters, n_subsets=info.n_subsets, best_iter=info.best_iter,
                best_root=info.best_root, n_inliers=info.n_inliers, best_median=info.best_median,
                F=np.array(info.F[:], np.float64).reshape(3, 3), stream_us=info.stream_us)


class FundamentalRansac(A.Owned):
    """cv::findFundamentalMat(pts1, pts2, FM_RANSAC, threshold, confidence, max_iters, mask) on the GPU.  One handle
    serves calls of up to max_points correspondences."""
    _destroy = "lvi_fmat_destroy"

    def __init__(self, lib, device=0, max_points=2048, max_iters=1000):
        self.lib = bind(lib)
        self.max_points = int(max_points)
        self.max_iters = int(max_iters)
        self._h = C.c_void_p()
        lib.check(lib.dll.lvi_fmat_create(int(device), self.max_points, self.max_iters, C.byref(self._h)), "lvi_fmat_create")

    def set_check_subset(self, mode):
        """1 (default): getSubset rejects subsets with collinear points in either set; 0: it does not"""
        self.lib.check(self.lib.dll.lvi_fmat_set_check_subset(self._h, int(mode)), "lvi_fmat_set_check_subset")

    def find(self, pts1, pts2, threshold=1.0, confidence=0.99, with_info=False):
        """pts1, pts2 [n, 2] (f32) -> status [n] uint8 (and the info dict)"""
        a = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
        if len(a) != len(b):
            raise ValueError("pts1 and pts2 differ in length")
        st = np.zeros(max(len(a), 1), np.uint8)
        info = FmatInfo()
        self.lib.check(self.lib.dll.lvi_fmat_find(self._h, A._ptr(a), A._ptr(b), len(a), float(threshold), float(confidence), A._ptr(st),
                                                  C.byref(info)), "lvi_fmat_find")
        st = st[:len(a)].copy()
        return (st, _info_dict(info)) if with_info else st

    def trace(self):
        """the last find's hypotheses: subsets [m, 7], nmodels [m], F [m, 3, 3, 3], score [m, 3] (inlier count for RANSAC,
        the median error as f32 bits for LMeDS)"""
        m = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_fmat_trace(self._h, None, None, None, None, 0, C.byref(m)), "lvi_fmat_trace")
        k = max(m.value, 1)
        sub = np.zeros((k, 7), np.int32); nm = np.zeros(k, np.int32); F = np.zeros((k, 3, 3, 3), np.float64); sc = np.zeros((k, 3), np.int32)
        self.lib.check(self.lib.dll.lvi_fmat_trace(self._h, A._ptr(sub), A._ptr(nm), A._ptr(F), A._ptr(sc), m.value, C.byref(m)), "lvi_fmat_trace")
        n = m.value
        return dict(subsets=sub[:n].copy(), nmodels=nm[:n].copy(), F=F[:n].copy(), score=sc[:n].copy())
