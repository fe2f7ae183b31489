"""Python handle over include/lvi_loop.h: mapOptimization's loop-closure registration (performLoopClosure,
mapOptimization.cpp:549-628: the two submaps of loopFindNearKeyframes and the ICP between them) over the device
keyframe store of a lidar handle.

A separate ABI from include/lvi_hotpath.h: only the product library exports it, so its signature table lives here and
is bound against ``liblvi_hip.so`` alone."""
import ctypes as C

import numpy as np

from . import _abi as A

_P = C.POINTER
_vp, _i32, _i64, _f32, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double

SOURCE, TARGET, ALIGNED = 0, 1, 2
OK, TOO_FEW_POINTS, NO_CORRESPONDENCES = 0, 1, 2
CONV_NOT_CONVERGED, CONV_ITERATIONS, CONV_TRANSFORM, CONV_ABS_MSE, CONV_REL_MSE, CONV_NO_CORRESPONDENCES = range(6)
MAX_POINTS = 1 << 24
N_SUMS = 17


class LoopParams(C.Structure):
    _fields_ = [("search_num", _i32), ("leaf", _f32), ("max_corr_dist", _f32), ("max_iters", _i32), ("transformation_epsilon", _f64),
                ("fitness_epsilon", _f64), ("min_source", _i32), ("min_target", _i32), ("incremental_cloud", _i32)]


class LoopInfo(C.Structure):
    _fields_ = [("status", _i32), ("n_source", _i32), ("n_target", _i32), ("n_source_fused", _i32), ("n_target_fused", _i32),
                ("overflow_source", _i32), ("overflow_target", _i32), ("iterations", _i32), ("converged", _i32), ("convergence_state", _i32),
                ("n_corr", _i32), ("key_cur", _i32), ("key_pre", _i32), ("transformation", _f32 * 16), ("fitness", _f64), ("mse", _f64)]


# name -> (restype, argtypes), one entry per function of include/lvi_loop.h
LOOP_SIGNATURES = {
    "lvi_loop_abi_version": (_i32, []),
    "lvi_loop_params_default": (None, [_P(LoopParams)]),
    "lvi_loop_reserve": (_i32, [_vp, _i32, _i32]),
    "lvi_loop_release": (_i32, [_vp]),
    "lvi_loop_arena_bytes": (_i32, [_vp, _P(_i64)]),
    "lvi_loop_start": (_i32, [_vp, _i32, _i32, _P(LoopParams)]),
    "lvi_loop_result": (_i32, [_vp, _P(LoopInfo)]),
    "lvi_loop_fetch": (_i32, [_vp, _i32, _i32, _i32, _vp]),
    "lvi_loop_debug_step": (_i32, [_vp, _vp, _vp, _vp, _vp]),
}


def bind(lib):
    """set the loop-closure signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(LOOP_SIGNATURES)


class LoopIcp:
    """the loop-closure calls of one lidar handle (a LidarHotpath, or the handle a SequentialMapper owns).  result() and
    fetch() may run on another thread while the owner runs scans; start / debug_step / reserve / release may not
    (include/lvi_loop.h)."""

    def __init__(self, lidar_handle):
        self.lib = bind(lidar_handle.lib)
        self.lidar = lidar_handle
        self._h = lidar_handle._h

    def default_params(self, **kw):
        p = LoopParams()
        self.lib.dll.lvi_loop_params_default(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        return p

    def reserve(self, max_source_points, max_target_points):
        self.lib.check(self.lib.dll.lvi_loop_reserve(self._h, int(max_source_points), int(max_target_points)), "lvi_loop_reserve")

    def release(self):
        self.lib.check(self.lib.dll.lvi_loop_release(self._h), "lvi_loop_release")

    def arena_bytes(self):
        b = _i64(0)
        self.lib.check(self.lib.dll.lvi_loop_arena_bytes(self._h, C.byref(b)), "lvi_loop_arena_bytes")
        return b.value

    def start(self, key_cur, key_pre, params=None, **kw):
        """enqueue the whole job (submaps, index, ICP, fitness) without waiting for the GPU"""
        p = params if params is not None else self.default_params(**kw)
        self.lib.check(self.lib.dll.lvi_loop_start(self._h, int(key_cur), int(key_pre), C.byref(p)), "lvi_loop_start")

    def result(self):
        r = LoopInfo()
        self.lib.check(self.lib.dll.lvi_loop_result(self._h, C.byref(r)), "lvi_loop_result")
        d = {k: getattr(r, k) for k, _ in LoopInfo._fields_ if k != "transformation"}
        d["converged"] = bool(d["converged"])
        d["transformation"] = np.array(r.transformation, np.float32).reshape(4, 4)
        return d

    def fetch(self, what=ALIGNED, first=0, count=None):
        """points [first, first + count) of the filtered source / target or the aligned source of the last job"""
        if count is None:
            r = self.result()
            count = (r["n_target"] if what == TARGET else r["n_source"]) - int(first)
        out = np.zeros(max(int(count), 1), A.PT_DTYPE)
        self.lib.check(self.lib.dll.lvi_loop_fetch(self._h, int(what), int(first), int(count), A._ptr(out)), "lvi_loop_fetch")
        return out[:int(count)]

    def debug_step(self, T):
        """one correspondence pass of the last job's clouds under T (4x4): (nn_idx, nn_sqd, sums[17])"""
        n = self.result()["n_source"]
        T = np.ascontiguousarray(T, np.float32).reshape(16)
        idx = np.zeros(max(n, 1), np.int32); sqd = np.zeros(max(n, 1), np.float32); sums = np.zeros(N_SUMS, np.float64)
        self.lib.check(self.lib.dll.lvi_loop_debug_step(self._h, A._ptr(T), A._ptr(idx), A._ptr(sqd), A._ptr(sums)), "lvi_loop_debug_step")
        return idx[:n], sqd[:n], sums
