"""Python handle over include/lvi_fman.h: vins_estimator's FeatureManager (feature_manager.{h,cpp}: addFeatureCheckParallax,
triangulate, the depth vector, the three slide operations, getCorresponding) and the factor loops of Estimator::optimization
(estimator.cpp:745-789, :849-889) over a feature table resident on the GPU — DESIGN §26.

A separate ABI from include/lvi_hotpath.h: only the product library exports it, so its signature table lives here and is
bound against ``liblvi_hip.so`` alone.  The projection record is the marginalisation's."""
import ctypes as C

import numpy as np

from . import _abi as A
from ._abi import _arr, _d
from .marg import PROJECTION_DTYPE

_P = C.POINTER
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double

MAX_FEATURES, WINDOW, MAX_OBS, MAX_SWEEPS = 4096, 10, 11, 30
MODE_WINDOW, MODE_MARG_OLD = 0, 1
# VinsMarginalizer::ID_* of host/lvi_marg_host.hpp
ID_POSE, ID_EX, ID_TD, ID_FEATURE = 0, 32, 33, 64


class FmanParams(C.Structure):
    _fields_ = [("init_depth", _f64), ("min_parallax", _f64)]


class FmanFrameInfo(C.Structure):
    _fields_ = [("last_track_num", _i32), ("parallax_num", _i32), ("keyframe", _i32), ("added", _i32), ("parallax_sum", _f64)]


class FmanTriInfo(C.Structure):
    _fields_ = [("triangulated", _i32), ("non_finite", _i32), ("negative", _i32), ("max_sweeps", _i32)]


class FmanIds(C.Structure):
    _fields_ = [("pose", _i32), ("ex", _i32), ("td", _i32), ("feature", _i32)]


# the numpy views of lvi_fman_obs and lvi_fman_feature
OBS_DTYPE = np.dtype([("point", "<f8", 3), ("uv", "<f8", 2), ("velocity", "<f8", 2), ("depth", "<f8"), ("cur_td", "<f8")])
FEATURE_DTYPE = np.dtype([("feature_id", "<i4"), ("start_frame", "<i4"), ("n_obs", "<i4"), ("lidar_depth_flag", "<i4"), ("solve_flag", "<i4"), ("reserved", "<i4"),
                          ("estimated_depth", "<f8"), ("obs", OBS_DTYPE, MAX_OBS)])
assert OBS_DTYPE.itemsize == 72 and FEATURE_DTYPE.itemsize == 824

# name -> (restype, argtypes), one entry per function of include/lvi_fman.h
FMAN_SIGNATURES = {
    "lvi_fman_abi_version": (_i32, []),
    "lvi_fman_params_default": (None, [_P(FmanParams)]),
    "lvi_fman_create": (_i32, [_i32, _i32, _P(_vp)]),
    "lvi_fman_destroy": (None, [_vp]),
    "lvi_fman_set_params": (_i32, [_vp, _P(FmanParams)]),
    "lvi_fman_clear": (_i32, [_vp]),
    "lvi_fman_count": (_i32, [_vp, _P(_i32), _P(_i32)]),
    "lvi_fman_add_frame": (_i32, [_vp, _i32, _i32, _P(_i32), _P(_f64), _f64, _P(FmanFrameInfo)]),
    "lvi_fman_triangulate": (_i32, [_vp, _P(_f64), _P(_f64), _P(_f64), _P(_f64), _P(FmanTriInfo)]),
    "lvi_fman_get_depth_vector": (_i32, [_vp, _i32, _P(_i32), _P(_f64)]),
    "lvi_fman_set_depth": (_i32, [_vp, _i32, _P(_f64)]),
    "lvi_fman_clear_depth": (_i32, [_vp, _i32, _P(_f64)]),
    "lvi_fman_remove_failures": (_i32, [_vp]),
    "lvi_fman_remove_back_shift_depth": (_i32, [_vp, _P(_f64), _P(_f64), _P(_f64), _P(_f64)]),
    "lvi_fman_remove_back": (_i32, [_vp]),
    "lvi_fman_remove_front": (_i32, [_vp, _i32]),
    "lvi_fman_corresponding": (_i32, [_vp, _i32, _i32, _i32, _P(_i32), _P(_f64)]),
    "lvi_fman_projections": (_i32, [_vp, _i32, _P(FmanIds), _i32, _P(_i32), _vp, _i32, _P(_i32), _P(_f64), _P(_i32)]),
    "lvi_fman_download": (_i32, [_vp, _i32, _P(_i32), _vp]),
}


def bind(lib):
    """set the feature-table signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(FMAN_SIGNATURES)


def _i(a):
    return a.ctypes.data_as(_P(_i32))


def _fields(s):
    return {k: getattr(s, k) for k, _ in s._fields_}


class FeatureTable(A.Owned):
    """f_manager: the feature list of one estimator, resident on the device in the reference's list order"""
    _destroy = "lvi_fman_destroy"
    feature_dtype = FEATURE_DTYPE
    record_dtype = PROJECTION_DTYPE

    def __init__(self, lib, device=0, max_features=1024, handle=None, **params):
        self.lib = bind(lib)
        self.max_features = int(max_features)
        self._own = handle is None                      # a view of a handle the host mirror owns is never destroyed from here
        self._h = C.c_void_p(handle) if handle is not None else C.c_void_p()
        if self._own:
            lib.check(lib.dll.lvi_fman_create(int(device), self.max_features, C.byref(self._h)), "lvi_fman_create")
        self.params = FmanParams()
        lib.dll.lvi_fman_params_default(C.byref(self.params))
        if params:
            self.set_params(**params)

    def _call(self, name, *args):
        return self.lib.check(getattr(self.lib.dll, name)(self._h, *args), name)

    def set_params(self, **kw):
        """init_depth, min_parallax"""
        p = FmanParams.from_buffer_copy(self.params)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(f"lvi_fman_params has no field {k}")
            setattr(p, k, v)
        self._call("lvi_fman_set_params", C.byref(p))
        self.params = p

    def clear(self):
        """clearState"""
        self._call("lvi_fman_clear")

    def count(self):
        """-> (feature.size(), getFeatureCount())"""
        a, b = C.c_int32(0), C.c_int32(0)
        self._call("lvi_fman_count", C.byref(a), C.byref(b))
        return a.value, b.value

    def add_frame(self, frame_count, ids, obs, td=0.0):
        """addFeatureCheckParallax: ids [n] strictly ascending, obs [n, 8] = x y z u v vx vy depth
        -> dict(last_track_num, parallax_num, keyframe, added, parallax_sum)"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        obs = _arr(np.asarray(obs, np.float64).reshape(-1, 8), (len(ids), 8))
        info = FmanFrameInfo()
        self._call("lvi_fman_add_frame", int(frame_count), len(ids), _i(ids), _d(obs), float(td), C.byref(info))
        return _fields(info)

    def triangulate(self, Ps, Rs, tic, ric):
        """triangulate: Ps [11, 3], Rs [11, 3, 3], tic [3], ric [3, 3] -> dict(triangulated, non_finite, negative, max_sweeps)"""
        Ps, Rs, tic, ric = _arr(Ps, (MAX_OBS, 3)), _arr(Rs, (MAX_OBS, 3, 3)), _arr(tic, (3,)), _arr(ric, (3, 3))
        info = FmanTriInfo()
        self._call("lvi_fman_triangulate", _d(Ps), _d(Rs), _d(tic), _d(ric), C.byref(info))
        return _fields(info)

    def depth_vector(self):
        """getDepthVector"""
        dep = np.zeros(max(1, self.count()[1]))
        n = C.c_int32(0)
        self._call("lvi_fman_get_depth_vector", len(dep), C.byref(n), _d(dep))
        return dep[:n.value].copy()

    def set_depth(self, x):
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        self._call("lvi_fman_set_depth", len(x), _d(x))

    def clear_depth(self, x):
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        self._call("lvi_fman_clear_depth", len(x), _d(x))

    def remove_failures(self):
        self._call("lvi_fman_remove_failures")

    def remove_back_shift_depth(self, marg_R, marg_P, new_R, new_P):
        a, b, c, d = _arr(marg_R, (3, 3)), _arr(marg_P, (3,)), _arr(new_R, (3, 3)), _arr(new_P, (3,))
        self._call("lvi_fman_remove_back_shift_depth", _d(a), _d(b), _d(c), _d(d))

    def remove_back(self):
        self._call("lvi_fman_remove_back")

    def remove_front(self, frame_count=WINDOW):
        self._call("lvi_fman_remove_front", int(frame_count))

    def corresponding(self, frame_l, frame_r):
        """getCorresponding -> [count, 2, 3]"""
        pairs = np.zeros((max(1, self.count()[0]), 2, 3))
        n = C.c_int32(0)
        self._call("lvi_fman_corresponding", int(frame_l), int(frame_r), len(pairs), C.byref(n), _d(pairs))
        return pairs[:n.value].copy()

    def projections(self, mode=MODE_WINDOW, estimate_td=True, ids=None):
        """-> dict(records [count] of record_dtype, inv_dep [n_features], lidar_flags [n_features]); ids: (pose, ex, td, feature)
        bases, by default VinsMarginalizer's with td = -1 when estimate_td is off"""
        b = FmanIds(*(ids if ids is not None else (ID_POSE, ID_EX, ID_TD if estimate_td else -1, ID_FEATURE)))
        n, e = C.c_int32(0), C.c_int32(0)
        self._call("lvi_fman_projections", int(mode), C.byref(b), 0, C.byref(n), None, 0, C.byref(e), None, None)
        recs, inv, flags = np.zeros(max(1, n.value), PROJECTION_DTYPE), np.zeros(max(1, e.value)), np.zeros(max(1, e.value), np.int32)
        self._call("lvi_fman_projections", int(mode), C.byref(b), len(recs), None, recs.ctypes.data_as(_vp), len(inv), None, _d(inv), _i(flags))
        return dict(records=recs[:n.value].copy(), inv_dep=inv[:e.value].copy(), lidar_flags=flags[:e.value].copy())

    def download(self):
        """the whole table in list order, as an array of feature_dtype"""
        tab = np.zeros(max(1, self.count()[0]), FEATURE_DTYPE)
        n = C.c_int32(0)
        self._call("lvi_fman_download", len(tab), C.byref(n), tab.ctypes.data_as(_vp))
        return tab[:n.value].copy()
