"""Python handle over include/lvi_pgo.h and include/lvi_pgo_gps.h: mapOptimization's factor graph (addOdomFactor,
addGPSFactor's factor, addLoopFactor, isam->update, the estimate read-back and the marginal covariance that gates GPS;
mapOptimization.cpp:1414-1428, 1430-1507, 1509-1527, 1546-1599) on the GPU, as the minimiser of the same cost — a
restatement of GTSAM's conventions, DESIGN §18 and §19.

A separate ABI from include/lvi_hotpath.h: only the product library exports it, so its signature table lives here and
is bound against ``liblvi_hip.so`` alone."""
import ctypes as C

import numpy as np

from . import _abi as A

_P = C.POINTER
_vp, _i32, _f32 = C.c_void_p, C.c_int32, C.c_float

MAX_POSES, MAX_LOOPS, MAX_ITERS = 65536, 64, 64
NOT_CONVERGED = 1


class PgoParams(C.Structure):
    _fields_ = [("full_logmap", C.c_int32), ("max_iters", C.c_int32), ("conv_eps", C.c_double)]


class PgoInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("chi2_before", C.c_double), ("chi2_after", C.c_double), ("max_step", C.c_double)]


# name -> (restype, argtypes), one entry per function of include/lvi_pgo.h
PGO_SIGNATURES = {
    "lvi_pgo_abi_version": (_i32, []),
    "lvi_pgo_params_default": (None, [_P(PgoParams)]),
    "lvi_pgo_create": (_i32, [_i32, _i32, _i32, _P(_vp)]),
    "lvi_pgo_destroy": (None, [_vp]),
    "lvi_pgo_clear": (_i32, [_vp]),
    "lvi_pgo_set_params": (_i32, [_vp, _P(PgoParams)]),
    "lvi_pgo_count": (_i32, [_vp, _P(_i32), _P(_i32)]),
    "lvi_pgo_add_pose": (_i32, [_vp, _P(_f32), _P(_f32), _P(_i32)]),
    "lvi_pgo_add_loop": (_i32, [_vp, _i32, _i32, _P(C.c_double), _f32]),
    "lvi_pgo_solve": (_i32, [_vp, _P(PgoInfo)]),
    "lvi_pgo_get_poses": (_i32, [_vp, _i32, _i32, _vp, _vp]),
}


# the same for include/lvi_pgo_gps.h, a separate header with its own version
PGO_GPS_SIGNATURES = {
    "lvi_pgo_gps_abi_version": (_i32, []),
    "lvi_pgo_gps_add": (_i32, [_vp, _i32, _P(_f32), _P(_f32)]),
    "lvi_pgo_gps_count": (_i32, [_vp, _P(_i32)]),
    "lvi_pgo_gps_marginal_covariance": (_i32, [_vp, _i32, _P(C.c_double)]),
}


def bind(lib):
    """set the pgo signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    lib.bind(PGO_SIGNATURES)
    return lib.bind(PGO_GPS_SIGNATURES)


def _pose6(p):
    return (C.c_float * 6)(*[float(v) for v in np.asarray(p, np.float32).reshape(6)])


class PoseGraph(A.Owned):
    """the keyframe pose graph: a prior on key 0, one odometry edge per later key, up to max_loops loop edges.  Poses
    are (roll, pitch, yaw, x, y, z)."""
    _destroy = "lvi_pgo_destroy"

    def __init__(self, lib, device=0, max_poses=4096, max_loops=MAX_LOOPS, **params):
        self.lib = bind(lib)
        self.max_poses, self.max_loops = int(max_poses), int(max_loops)
        self._h = C.c_void_p()
        lib.check(lib.dll.lvi_pgo_create(int(device), self.max_poses, self.max_loops, C.byref(self._h)), "lvi_pgo_create")
        self.params = PgoParams()
        lib.dll.lvi_pgo_params_default(C.byref(self.params))
        if params:
            self.set_params(**params)

    def set_params(self, **kw):
        """full_logmap (1 / 0), max_iters, conv_eps"""
        p = PgoParams(self.params.full_logmap, self.params.max_iters, self.params.conv_eps)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(f"lvi_pgo_params has no field {k}")
            setattr(p, k, v)
        self.lib.check(self.lib.dll.lvi_pgo_set_params(self._h, C.byref(p)), "lvi_pgo_set_params")
        self.params = p

    def clear(self):
        self.lib.check(self.lib.dll.lvi_pgo_clear(self._h), "lvi_pgo_clear")

    def count(self):
        n, l = C.c_int32(0), C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_pgo_count(self._h, C.byref(n), C.byref(l)), "lvi_pgo_count")
        return n.value, l.value

    def add_pose(self, pose_from, pose_to):
        """the prior (first call; pose_from may be None) or BetweenFactor(n - 1, n, poseFrom.between(poseTo)) -> the key's index"""
        idx = C.c_int32(-1)
        self.lib.check(self.lib.dll.lvi_pgo_add_pose(self._h, _pose6(pose_from) if pose_from is not None else None, _pose6(pose_to), C.byref(idx)),
                       "lvi_pgo_add_pose")
        return idx.value

    def add_loop(self, frm, to, between, variance):
        b = np.ascontiguousarray(between, np.float64).reshape(16)
        self.lib.check(self.lib.dll.lvi_pgo_add_loop(self._h, int(frm), int(to), b.ctypes.data_as(_P(C.c_double)), float(variance)), "lvi_pgo_add_loop")

    def add_gps(self, key, xyz, variance):
        """GPSFactor(key, xyz, Variances(variance)) (mapOptimization.cpp:1497-1499); the variances are taken as they are"""
        z = (C.c_float * 3)(*[float(v) for v in np.asarray(xyz, np.float32).reshape(3)])
        v = (C.c_float * 3)(*[float(x) for x in np.asarray(variance, np.float32).reshape(3)])
        self.lib.check(self.lib.dll.lvi_pgo_gps_add(self._h, int(key), z, v), "lvi_pgo_gps_add")

    def gps_count(self):
        n = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_pgo_gps_count(self._h, C.byref(n)), "lvi_pgo_gps_count")
        return n.value

    def marginal_covariance(self, key):
        """isam->marginalCovariance(key) (:1591) at the current poses -> [6, 6] float64, tangent order rotation, translation"""
        c = np.zeros(36, np.float64)
        self.lib.check(self.lib.dll.lvi_pgo_gps_marginal_covariance(self._h, int(key), c.ctypes.data_as(_P(C.c_double))), "lvi_pgo_gps_marginal_covariance")
        return c.reshape(6, 6)

    def solve(self):
        """-> dict(status, iterations, converged, chi2_before, chi2_after, max_step); status NOT_CONVERGED is soft"""
        info = PgoInfo()
        st = self.lib.check(self.lib.dll.lvi_pgo_solve(self._h, C.byref(info)), "lvi_pgo_solve")
        return dict(status=st, iterations=info.iterations, converged=bool(info.converged), chi2_before=info.chi2_before, chi2_after=info.chi2_after,
                    max_step=info.max_step)

    def poses(self, first=0, count=None):
        """-> (T [count, 4, 4] float64, rpyxyz [count, 6] float32)"""
        if count is None:
            count = self.count()[0] - int(first)
        T = np.zeros((max(count, 1), 16), np.float64)
        p = np.zeros((max(count, 1), 6), np.float32)
        self.lib.check(self.lib.dll.lvi_pgo_get_poses(self._h, int(first), int(count), A._ptr(T), A._ptr(p)), "lvi_pgo_get_poses")
        return T[:count].reshape(-1, 4, 4).copy(), p[:count].copy()
