"""Python handle over include/lvi_marg.h: the marginalisation of vins_estimator's sliding window (MarginalizationInfo:
marginalization_factor.cpp:89-129, 174-318, with the factors of estimator.cpp:813-976) on the GPU — DESIGN §21.

A separate ABI from include/lvi_hotpath.h: only the product library exports it, so its signature table lives here and
is bound against ``liblvi_hip.so`` alone."""
import ctypes as C

import numpy as np

from . import _abi as A
from ._abi import _d

_P = C.POINTER
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double

MAX_BLOCKS, MAX_PROJECTIONS, MAX_DENSE_FACTORS, MAX_DENSE_ROWS, MAX_DROP_DIM, MAX_KEEP_DIM = 2048, 8192, 16, 256, 512, 256
MAX_BLOCK_SIZE, MAX_SWEEPS, SHARE = 16, 64, 128
LOSS_NONE, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2
EIG_NOT_CONVERGED, NOT_FINITE = 1, 2


class MargCaps(C.Structure):
    _fields_ = [("max_blocks", _i32), ("max_projections", _i32), ("max_dense_factors", _i32), ("max_dense_rows", _i32), ("max_drop_dim", _i32),
                ("max_keep_dim", _i32)]


class MargParams(C.Structure):
    _fields_ = [("loss_type", _i32), ("max_sweeps", _i32), ("loss_a", _f64), ("sqrt_info", _f64), ("tr_over_row", _f64), ("half_row", _f64), ("eps", _f64)]


class MargProjection(C.Structure):
    _fields_ = [("pose_i", _i32), ("pose_j", _i32), ("ex", _i32), ("feature", _i32), ("td", _i32), ("reserved", _i32),
                ("pts_i", _f64 * 3), ("pts_j", _f64 * 3), ("velocity_i", _f64 * 2), ("velocity_j", _f64 * 2), ("td_i", _f64), ("td_j", _f64),
                ("row_i", _f64), ("row_j", _f64)]


class MargInfo(C.Structure):
    _fields_ = [("m", _i32), ("n", _i32), ("rank", _i32), ("rank_mm", _i32), ("sweeps_mm", _i32), ("sweeps_rr", _i32), ("flags", _i32), ("kept_blocks", _i32),
                ("cost", _f64), ("off_mm", _f64), ("off_rr", _f64)]


# the numpy view of an array of lvi_marg_projection
PROJECTION_DTYPE = np.dtype([("pose_i", "<i4"), ("pose_j", "<i4"), ("ex", "<i4"), ("feature", "<i4"), ("td", "<i4"), ("reserved", "<i4"),
                             ("pts_i", "<f8", 3), ("pts_j", "<f8", 3), ("velocity_i", "<f8", 2), ("velocity_j", "<f8", 2), ("td_i", "<f8"), ("td_j", "<f8"),
                             ("row_i", "<f8"), ("row_j", "<f8")])

# name -> (restype, argtypes), one entry per function of include/lvi_marg.h
MARG_SIGNATURES = {
    "lvi_marg_abi_version": (_i32, []),
    "lvi_marg_params_default": (None, [_P(MargParams)]),
    "lvi_marg_create": (_i32, [_i32, _P(MargCaps), _P(_vp)]),
    "lvi_marg_destroy": (None, [_vp]),
    "lvi_marg_clear": (_i32, [_vp]),
    "lvi_marg_set_params": (_i32, [_vp, _P(MargParams)]),
    "lvi_marg_begin": (_i32, [_vp]),
    "lvi_marg_set_block": (_i32, [_vp, _i32, _i32, _P(_f64)]),
    "lvi_marg_add_projection": (_i32, [_vp, _i32, _vp]),
    "lvi_marg_add_dense": (_i32, [_vp, _i32, _i32, _P(_i32), _P(_f64), _P(_f64), _P(_i32)]),
    "lvi_marg_add_last_prior": (_i32, [_vp, _i32, _P(_i32)]),
    "lvi_marg_marginalize": (_i32, [_vp, _P(MargInfo)]),
    "lvi_marg_get_layout": (_i32, [_vp, _P(MargInfo), _i32, _P(_i32), _P(_i32), _P(_i32), _P(_i32), _P(_f64)]),
    "lvi_marg_get_prior": (_i32, [_vp, _P(_f64), _P(_f64)]),
    "lvi_marg_remap": (_i32, [_vp, _P(_i32), _P(_i32), _i32]),
    "lvi_marg_debug_system": (_i32, [_vp, _i32, _P(_i32), _P(_f64), _P(_f64)]),
}


def bind(lib):
    """set the marg signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(MARG_SIGNATURES)


def _i(a):
    return a.ctypes.data_as(_P(_i32))


def _info(i):
    return {k: getattr(i, k) for k, _ in MargInfo._fields_}


class Marginalizer(A.Owned):
    """one sliding window's MarginalizationInfo; the prior it computes stays on the device for the next call"""
    _destroy = "lvi_marg_destroy"
    record_dtype = PROJECTION_DTYPE

    def __init__(self, lib, device=0, max_blocks=256, max_projections=2048, max_dense_factors=2, max_dense_rows=32, max_drop_dim=256, max_keep_dim=128,
                 handle=None, **params):
        self.lib = bind(lib)
        self.caps = MargCaps(int(max_blocks), int(max_projections), int(max_dense_factors), int(max_dense_rows), int(max_drop_dim), int(max_keep_dim))
        self._own = handle is None
        self._h = C.c_void_p(handle) if handle is not None else C.c_void_p()
        if self._own:
            lib.check(lib.dll.lvi_marg_create(int(device), C.byref(self.caps), C.byref(self._h)), "lvi_marg_create")
        self.params = MargParams()
        lib.dll.lvi_marg_params_default(C.byref(self.params))
        if params:
            self.set_params(**params)

    def set_params(self, **kw):
        """loss_type, max_sweeps, loss_a, sqrt_info, tr_over_row, half_row, eps"""
        p = MargParams.from_buffer_copy(self.params)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(f"lvi_marg_params has no field {k}")
            setattr(p, k, v)
        self.lib.check(self.lib.dll.lvi_marg_set_params(self._h, C.byref(p)), "lvi_marg_set_params")
        self.params = p

    def clear(self):
        self.lib.check(self.lib.dll.lvi_marg_clear(self._h), "lvi_marg_clear")

    def begin(self):
        self.lib.check(self.lib.dll.lvi_marg_begin(self._h), "lvi_marg_begin")

    def set_block(self, bid, values, size=None):
        v = np.ascontiguousarray(values, np.float64).reshape(-1)
        self.lib.check(self.lib.dll.lvi_marg_set_block(self._h, int(bid), int(len(v) if size is None else size), _d(v)), "lvi_marg_set_block")

    def add_projection(self, records):
        """records: a PROJECTION_DTYPE array, one ProjectionTdFactor (td >= 0) or ProjectionFactor (td == -1) each"""
        r = np.ascontiguousarray(records, PROJECTION_DTYPE).reshape(-1)
        self.lib.check(self.lib.dll.lvi_marg_add_projection(self._h, len(r), r.ctypes.data_as(_vp) if len(r) else None), "lvi_marg_add_projection")

    def add_dense(self, ids, residual, jacobians, drop):
        """jacobians: one [n_rows, size of the block] array per block, as ceres fills them"""
        ids = np.ascontiguousarray(ids, np.int32)
        r = np.ascontiguousarray(residual, np.float64).reshape(-1)
        J = np.concatenate([np.ascontiguousarray(j, np.float64).reshape(len(r), -1).ravel() for j in jacobians])
        mask = np.ascontiguousarray(drop, np.int32)
        self.lib.check(self.lib.dll.lvi_marg_add_dense(self._h, len(r), len(ids), _i(ids), _d(r), _d(J), _i(mask)), "lvi_marg_add_dense")

    def add_last_prior(self, drop_ids):
        d = np.ascontiguousarray(drop_ids, np.int32).reshape(-1)
        self.lib.check(self.lib.dll.lvi_marg_add_last_prior(self._h, len(d), _i(d) if len(d) else None), "lvi_marg_add_last_prior")

    def marginalize(self):
        """-> dict(status, m, n, rank, ...); status EIG_NOT_CONVERGED and NOT_FINITE are soft"""
        info = MargInfo()
        st = self.lib.check(self.lib.dll.lvi_marg_marginalize(self._h, C.byref(info)), "lvi_marg_marginalize")
        return dict(status=st, **_info(info))

    def layout(self):
        """-> dict(info, ids, sizes, idx, values): the kept blocks, the reference's keep_block_size / idx / data"""
        info, n = MargInfo(), C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_marg_get_layout(self._h, C.byref(info), 0, C.byref(n), None, None, None, None), "lvi_marg_get_layout")
        k = n.value
        ids, sizes, idx, vals = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros((k, MAX_BLOCK_SIZE), np.float64)
        self.lib.check(self.lib.dll.lvi_marg_get_layout(self._h, None, k, None, _i(ids), _i(sizes), _i(idx), _d(vals)), "lvi_marg_get_layout")
        return dict(info=_info(info), ids=ids, sizes=sizes, idx=idx, values=[vals[j, :sizes[j]].copy() for j in range(k)])

    def prior(self):
        """-> (linearized_jacobians [n, n], linearized_residuals [n])"""
        n = self.layout()["info"]["n"]
        J, r = np.zeros((n, n), np.float64), np.zeros(n, np.float64)
        self.lib.check(self.lib.dll.lvi_marg_get_prior(self._h, _d(J), _d(r)), "lvi_marg_get_prior")
        return J, r

    def remap(self, old_ids, new_ids):
        a, b = np.ascontiguousarray(old_ids, np.int32), np.ascontiguousarray(new_ids, np.int32)
        assert len(a) == len(b)
        self.lib.check(self.lib.dll.lvi_marg_remap(self._h, _i(a), _i(b), len(a)), "lvi_marg_remap")

    def debug_system(self):
        """-> (A [m + n, m + n], b [m + n]) of the last marginalize, before the Schur step"""
        n = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_marg_debug_system(self._h, 0, C.byref(n), None, None), "lvi_marg_debug_system")
        pos = n.value
        A, b = np.zeros((pos, pos), np.float64), np.zeros(pos, np.float64)
        self.lib.check(self.lib.dll.lvi_marg_debug_system(self._h, pos, None, _d(A), _d(b)), "lvi_marg_debug_system")
        return A, b
