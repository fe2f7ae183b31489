"""Python handle over include/lvi_win.h: the solve of vins_estimator's sliding window (estimator.cpp:696-811: the problem
build, ceres::Solve with DENSE_SCHUR + DOGLEG, the write-back) on the GPU — DESIGN §22.

A separate ABI from include/lvi_hotpath.h and include/lvi_marg.h: only the product library exports it, so its signature
table lives here and is bound against ``liblvi_hip.so`` alone.  The projection record is the marginalisation's."""
import ctypes as C

import numpy as np

from . import _abi as A
from ._abi import _d
from .marg import PROJECTION_DTYPE, MargProjection  # noqa: F401

_P = C.POINTER
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double

MAX_BLOCKS, MAX_PROJECTIONS, MAX_ELIMINATED, MAX_IMU, MAX_PRIOR_ROWS, MAX_DIM = 4096, 8192, 2048, 16, 256, 256
MAX_BLOCK_SIZE, MAX_ITERATIONS, SHARE, CHOL_BLOCK = 16, 64, 128, 32
CONSTANT, ELIMINATED = 1, 2
NOT_FINITE, BAD_COVARIANCE = 1, 2
TERM_NONE, TERM_FUNCTION, TERM_GRADIENT, TERM_PARAMETER, TERM_ITERATIONS, TERM_TIME, TERM_RADIUS, TERM_INVALID_STEPS = range(8)
STEP_NONE, STEP_GAUSS_NEWTON, STEP_CAUCHY, STEP_INTERPOLATED = range(4)


class WinCaps(C.Structure):
    _fields_ = [("max_blocks", _i32), ("max_projections", _i32), ("max_eliminated", _i32), ("max_imu", _i32), ("max_prior_rows", _i32), ("max_dim", _i32)]


class WinParams(C.Structure):
    _fields_ = [("loss_type", _i32), ("max_iterations", _i32), ("jacobi_scaling", _i32), ("max_invalid_steps", _i32),
                ("loss_a", _f64), ("sqrt_info", _f64), ("tr_over_row", _f64), ("half_row", _f64), ("G", _f64 * 3), ("max_time_s", _f64),
                ("initial_radius", _f64), ("max_radius", _f64), ("min_radius", _f64), ("min_relative_decrease", _f64), ("function_tolerance", _f64),
                ("gradient_tolerance", _f64), ("parameter_tolerance", _f64), ("initial_mu", _f64), ("min_mu", _f64), ("max_mu", _f64),
                ("mu_increase_factor", _f64), ("increase_threshold", _f64), ("decrease_threshold", _f64), ("min_diagonal", _f64), ("max_diagonal", _f64)]


class WinImu(C.Structure):
    _fields_ = [("pose_i", _i32), ("speed_bias_i", _i32), ("pose_j", _i32), ("speed_bias_j", _i32), ("sum_dt", _f64), ("delta_p", _f64 * 3),
                ("delta_q", _f64 * 4), ("delta_v", _f64 * 3), ("linearized_ba", _f64 * 3), ("linearized_bg", _f64 * 3), ("jacobian", _f64 * 225),
                ("covariance", _f64 * 225)]


class WinInfo(C.Structure):
    _fields_ = [("iterations", _i32), ("successful_steps", _i32), ("termination", _i32), ("flags", _i32), ("dim", _i32), ("eliminated", _i32),
                ("initial_cost", _f64), ("final_cost", _f64), ("radius", _f64), ("mu", _f64), ("time_s", _f64)]


class WinIteration(C.Structure):
    _fields_ = [("iteration", _i32), ("step_kind", _i32), ("accepted", _i32), ("mu_retries", _i32), ("cost", _f64), ("cost_change", _f64),
                ("model_cost_change", _f64), ("rho", _f64), ("gradient_max_norm", _f64), ("step_norm", _f64), ("radius", _f64), ("mu", _f64),
                ("gauss_newton_norm", _f64), ("cauchy_norm", _f64)]


# the numpy view of an array of lvi_win_imu
IMU_DTYPE = np.dtype([("pose_i", "<i4"), ("speed_bias_i", "<i4"), ("pose_j", "<i4"), ("speed_bias_j", "<i4"), ("sum_dt", "<f8"), ("delta_p", "<f8", 3),
                      ("delta_q", "<f8", 4), ("delta_v", "<f8", 3), ("linearized_ba", "<f8", 3), ("linearized_bg", "<f8", 3), ("jacobian", "<f8", (15, 15)),
                      ("covariance", "<f8", (15, 15))])

# name -> (restype, argtypes), one entry per function of include/lvi_win.h
WIN_SIGNATURES = {
    "lvi_win_abi_version": (_i32, []),
    "lvi_win_params_default": (None, [_P(WinParams)]),
    "lvi_win_create": (_i32, [_i32, _P(WinCaps), _P(_vp)]),
    "lvi_win_destroy": (None, [_vp]),
    "lvi_win_set_params": (_i32, [_vp, _P(WinParams)]),
    "lvi_win_begin": (_i32, [_vp]),
    "lvi_win_set_block": (_i32, [_vp, _i32, _i32, _P(_f64), _i32]),
    "lvi_win_add_projection": (_i32, [_vp, _i32, _vp]),
    "lvi_win_add_imu": (_i32, [_vp, _i32, _vp]),
    "lvi_win_set_prior_from_marg": (_i32, [_vp, _vp]),
    "lvi_win_set_prior": (_i32, [_vp, _i32, _P(_f64), _P(_f64), _i32, _P(_i32), _P(_i32), _P(_i32), _P(_f64)]),
    "lvi_win_solve": (_i32, [_vp, _P(WinInfo)]),
    "lvi_win_get_block": (_i32, [_vp, _i32, _P(_f64)]),
    "lvi_win_get_log": (_i32, [_vp, _i32, _P(_i32), _P(WinIteration)]),
    "lvi_win_debug_system": (_i32, [_vp, _i32, _i32, _i32, _i32, _P(_i32), _P(_i32), _P(_i32), _P(_f64), _P(_f64), _P(_f64), _P(_f64), _P(_f64), _P(_f64),
                                    _P(_f64), _P(_f64)]),
}


def bind(lib):
    """set the window-solve signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(WIN_SIGNATURES)


def _i(a):
    return a.ctypes.data_as(_P(_i32))


def _fields(s):
    return {k: (list(getattr(s, k)) if hasattr(getattr(s, k), "__len__") else getattr(s, k)) for k, _ in s._fields_}


class WindowSolver(A.Owned):
    """one sliding window's optimisation problem; the blocks hold the solution after solve()"""
    _destroy = "lvi_win_destroy"
    record_dtype = PROJECTION_DTYPE
    imu_dtype = IMU_DTYPE

    def __init__(self, lib, device=0, max_blocks=512, max_projections=2048, max_eliminated=512, max_imu=16, max_prior_rows=128, max_dim=256, **params):
        self.lib = bind(lib)
        self.caps = WinCaps(int(max_blocks), int(max_projections), int(max_eliminated), int(max_imu), int(max_prior_rows), int(max_dim))
        self._h = C.c_void_p()
        self._sizes, self._nproj = {}, 0
        lib.check(lib.dll.lvi_win_create(int(device), C.byref(self.caps), C.byref(self._h)), "lvi_win_create")
        self.params = WinParams()
        lib.dll.lvi_win_params_default(C.byref(self.params))
        if params:
            self.set_params(**params)

    def set_params(self, **kw):
        """any field of lvi_win_params; G takes three values"""
        p = WinParams.from_buffer_copy(self.params)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(f"lvi_win_params has no field {k}")
            setattr(p, k, (_f64 * 3)(*v) if k == "G" else v)
        self.lib.check(self.lib.dll.lvi_win_set_params(self._h, C.byref(p)), "lvi_win_set_params")
        self.params = p

    def begin(self):
        self.lib.check(self.lib.dll.lvi_win_begin(self._h), "lvi_win_begin")
        self._sizes, self._nproj = {}, 0

    def set_block(self, bid, values, flags=0, size=None):
        v = np.ascontiguousarray(values, np.float64).reshape(-1)
        n = int(len(v) if size is None else size)
        self.lib.check(self.lib.dll.lvi_win_set_block(self._h, int(bid), n, _d(v), int(flags)), "lvi_win_set_block")
        self._sizes[int(bid)] = n

    def add_projection(self, records):
        r = np.ascontiguousarray(records, PROJECTION_DTYPE).reshape(-1)
        self.lib.check(self.lib.dll.lvi_win_add_projection(self._h, len(r), r.ctypes.data_as(_vp) if len(r) else None), "lvi_win_add_projection")
        self._nproj += len(r)

    def add_imu(self, records):
        r = np.ascontiguousarray(records, IMU_DTYPE).reshape(-1)
        self.lib.check(self.lib.dll.lvi_win_add_imu(self._h, len(r), r.ctypes.data_as(_vp) if len(r) else None), "lvi_win_add_imu")

    def set_prior_from_marg(self, marginalizer):
        """the resident prior of a marg.Marginalizer on the same device: nothing crosses the bus"""
        self.lib.check(self.lib.dll.lvi_win_set_prior_from_marg(self._h, marginalizer._h), "lvi_win_set_prior_from_marg")

    def set_prior(self, J, r, ids, sizes, idx, values):
        """what Marginalizer.prior() and .layout() return; values: one array per kept block"""
        J, r = np.ascontiguousarray(J, np.float64), np.ascontiguousarray(r, np.float64)
        ids, sizes, idx = (np.ascontiguousarray(a, np.int32) for a in (ids, sizes, idx))
        vals = np.zeros((len(ids), MAX_BLOCK_SIZE), np.float64)
        for k, v in enumerate(values):
            vals[k, :len(v)] = v
        self.lib.check(self.lib.dll.lvi_win_set_prior(self._h, len(r), _d(J), _d(r), len(ids), _i(ids), _i(sizes), _i(idx), _d(vals)), "lvi_win_set_prior")

    def solve(self):
        """-> dict(status, iterations, termination, initial_cost, final_cost, ...); status NOT_FINITE and BAD_COVARIANCE are soft"""
        info = WinInfo()
        st = self.lib.check(self.lib.dll.lvi_win_solve(self._h, C.byref(info)), "lvi_win_solve")
        return dict(status=st, **_fields(info))

    def block(self, bid):
        v = np.zeros(MAX_BLOCK_SIZE, np.float64)
        self.lib.check(self.lib.dll.lvi_win_get_block(self._h, int(bid), _d(v)), "lvi_win_get_block")
        return v[:self._sizes[int(bid)]].copy()

    def log(self):
        """-> one dict per entry of the last solve's log, entry 0 the state it started from"""
        n = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_win_get_log(self._h, 0, C.byref(n), None), "lvi_win_get_log")
        arr = (WinIteration * max(1, n.value))()
        self.lib.check(self.lib.dll.lvi_win_get_log(self._h, n.value, None, arr), "lvi_win_get_log")
        return [_fields(arr[k]) for k in range(n.value)]

    def debug_system(self):
        """-> dict(H [D, D], g [D], hdiag [E], gf [E], W [E, D], proj_rows [P, 2, 21], dense [R, D + 1], cost, status) at the
        blocks' current values, before scaling and regularisation"""
        D, E, R = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        f = self.lib.dll.lvi_win_debug_system
        self.lib.check(f(self._h, 0, 0, 0, 0, C.byref(D), C.byref(E), C.byref(R), None, None, None, None, None, None, None, None), "lvi_win_debug_system")
        D, E, R, P = D.value, E.value, R.value, self._nproj
        H, g, hd, gf, W = np.zeros((D, D)), np.zeros(D), np.zeros(E), np.zeros(E), np.zeros((E, D))
        rows, dense, cost = np.zeros((P, 2, 21)), np.zeros((R, D + 1)), C.c_double(0)
        st = self.lib.check(f(self._h, D, E, P, R, None, None, None, _d(H), _d(g), _d(hd), _d(gf), _d(W), _d(rows), _d(dense), C.byref(cost)), "lvi_win_debug_system")
        return dict(H=H, g=g, hdiag=hd, gf=gf, W=W, proj_rows=rows, dense=dense, cost=cost.value, status=st)
