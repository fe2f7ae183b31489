"""Python handle over include/lvi_align.h: the visual-inertial alignment of vins_estimator's initialisation (tmp_pre_integration
and all_image_frame, estimator.cpp:99, :132-135, :1019-1033; the excitation check, :273-300; solveGyroscopeBias, RefineGravity,
LinearAlignment and VisualIMUAlignment, initial/initial_aligment.cpp:3-209; the tail of visualInitialAlign, estimator.cpp:
450-486) on the GPU — DESIGN §31.

A separate ABI from include/lvi_hotpath.h: only the product library exports it, so its signature table lives here and is
bound against ``liblvi_hip.so`` alone."""
import ctypes as C

import numpy as np

from . import _abi as A
from ._abi import _arr, _d

_P = C.POINTER
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double

MAX_FRAMES, SYSTEMS = 256, 5
OK, GRAVITY_NORM, NEGATIVE_SCALE, NEGATIVE_SCALE_REFINED, SINGULAR, TOO_FEW = range(6)
APPLY_OPPOSITE = 1


class AlignCaps(C.Structure):
    _fields_ = [("max_frames", _i32), ("max_samples", _i32)]


class AlignParams(C.Structure):
    _fields_ = [("acc_n", _f64), ("gyr_n", _f64), ("acc_w", _f64), ("gyr_w", _f64), ("G", _f64 * 3), ("TIC", _f64 * 3)]


class AlignInfo(C.Structure):
    _fields_ = [("ok", _i32), ("reason", _i32), ("n_state", _i32), ("frames", _i32), ("delta_bg", _f64 * 3), ("s", _f64), ("g_linear", _f64 * 3),
                ("g", _f64 * 3), ("min_pivot", _f64 * 6)]


class AlignFrame(C.Structure):
    _fields_ = [("stamp", _f64), ("R", _f64 * 9), ("T", _f64 * 3), ("is_key_frame", _i32), ("has_preintegration", _i32), ("samples", _i32), ("reserved", _i32),
                ("sum_dt", _f64), ("delta_p", _f64 * 3), ("delta_q", _f64 * 4), ("delta_v", _f64 * 3), ("linearized_ba", _f64 * 3), ("linearized_bg", _f64 * 3),
                ("linearized_acc", _f64 * 3), ("linearized_gyr", _f64 * 3), ("jacobian", _f64 * 225)]


# name -> (restype, argtypes), one entry per function of include/lvi_align.h
ALIGN_SIGNATURES = {
    "lvi_align_abi_version": (_i32, []),
    "lvi_align_params_default": (None, [_P(AlignParams)]),
    "lvi_align_create": (_i32, [_i32, _P(AlignCaps), _P(_vp)]),
    "lvi_align_destroy": (None, [_vp]),
    "lvi_align_set_params": (_i32, [_vp, _P(AlignParams)]),
    "lvi_align_clear": (_i32, [_vp]),
    "lvi_align_push_imu": (_i32, [_vp, _i32, _P(_f64), _P(_f64), _P(_f64)]),
    "lvi_align_add_frame": (_i32, [_vp, _f64, _P(_f64), _P(_f64)]),
    "lvi_align_erase_through": (_i32, [_vp, _f64]),
    "lvi_align_set_pose": (_i32, [_vp, _f64, _P(_f64), _P(_f64), _i32]),
    "lvi_align_frames": (_i32, [_vp, _P(_i32)]),
    "lvi_align_excitation": (_i32, [_vp, _P(_f64)]),
    "lvi_align_solve": (_i32, [_vp, _P(_f64), _P(_f64), _P(_f64), _i32, _P(AlignInfo)]),
    "lvi_align_get_frame": (_i32, [_vp, _i32, _P(AlignFrame), _i32, _P(_f64), _P(_f64), _P(_f64)]),
    "lvi_align_last_system": (_i32, [_vp, _i32, _P(_i32), _P(_f64), _P(_f64), _P(_f64), _i32]),
    "lvi_align_apply": (_i32, [_P(AlignParams), _i32, _P(_f64), _P(_f64), _P(_f64), _P(_f64), _i32, _P(_f64), _P(_f64), _i32, _P(_f64), _P(_i32)]),
}


def bind(lib):
    """set the alignment signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(ALIGN_SIGNATURES)


class ImuAligner(A.Owned):
    """all_image_frame with its per-image preintegrations and tmp_pre_integration, resident on the device"""
    _destroy = "lvi_align_destroy"

    def __init__(self, lib, device=0, max_frames=64, max_samples=2048, **params):
        self.lib = bind(lib)
        self.caps = AlignCaps(int(max_frames), int(max_samples))
        self._h = C.c_void_p()
        lib.check(lib.dll.lvi_align_create(int(device), C.byref(self.caps), C.byref(self._h)), "lvi_align_create")
        self.params = AlignParams()
        lib.dll.lvi_align_params_default(C.byref(self.params))
        if params:
            self.set_params(**params)

    def _call(self, name, *args):
        return self.lib.check(getattr(self.lib.dll, name)(self._h, *args), name)

    def set_params(self, **kw):
        """acc_n, gyr_n, acc_w, gyr_w, G (three values), TIC (three values)"""
        p = AlignParams.from_buffer_copy(self.params)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(f"lvi_align_params has no field {k}")
            setattr(p, k, (_f64 * 3)(*v) if k in ("G", "TIC") else v)
        self._call("lvi_align_set_params", C.byref(p))
        self.params = p

    def clear(self):
        """clearState"""
        self._call("lvi_align_clear")

    def push_imu(self, dt, acc, gyr):
        """estimator.cpp:99 for len(dt) samples"""
        dt = np.ascontiguousarray(dt, np.float64).reshape(-1)
        acc, gyr = _arr(np.asarray(acc, np.float64).reshape(-1, 3), (len(dt), 3)), _arr(np.asarray(gyr, np.float64).reshape(-1, 3), (len(dt), 3))
        self._call("lvi_align_push_imu", len(dt), _d(dt), _d(acc), _d(gyr))

    def add_frame(self, stamp, Ba, Bg):
        """:132-135"""
        self._call("lvi_align_add_frame", float(stamp), _d(_arr(Ba, (3,))), _d(_arr(Bg, (3,))))

    def erase_through(self, t0):
        """:1019-1033"""
        self._call("lvi_align_erase_through", float(t0))

    def set_pose(self, stamp, R, T, is_key_frame):
        self._call("lvi_align_set_pose", float(stamp), _d(_arr(R, (3, 3))), _d(_arr(T, (3,))), int(bool(is_key_frame)))

    def __len__(self):
        n = _i32(0)
        self._call("lvi_align_frames", C.byref(n))
        return n.value

    def excitation(self):
        """:273-300 -> var"""
        v = _f64(0.0)
        self._call("lvi_align_excitation", C.byref(v))
        return v.value

    def solve(self, Bgs):
        """VisualIMUAlignment -> (Bgs advanced [11, 3], info); info: ok, reason, n_state, frames, delta_bg, s, g_linear, g, x
        [n_state], min_pivot [6]"""
        Bgs = _arr(Bgs, (11, 3)).copy()
        cap = 3 * len(self) + 4
        g, x, info = np.zeros(3), np.zeros(cap), AlignInfo()
        self._call("lvi_align_solve", _d(Bgs), _d(g), _d(x), cap, C.byref(info))
        return Bgs, dict(ok=bool(info.ok), reason=info.reason, n_state=info.n_state, frames=info.frames, delta_bg=np.array(info.delta_bg), s=info.s,
                         g_linear=np.array(info.g_linear), g=g, x=x[:info.n_state].copy(), min_pivot=np.array(info.min_pivot))

    def frame(self, index):
        """-> dict(stamp, R [9], T [3], key, samples, pre: None or the preintegration's fields, dt, acc, gyr)"""
        f = AlignFrame()
        self._call("lvi_align_get_frame", int(index), C.byref(f), 0, None, None, None)
        n = f.samples
        dt, acc, gyr = np.zeros(max(1, n)), np.zeros((max(1, n), 3)), np.zeros((max(1, n), 3))
        self._call("lvi_align_get_frame", int(index), C.byref(f), len(dt), _d(dt), _d(acc), _d(gyr))
        pre = None
        if f.has_preintegration:
            pre = {k: np.array(getattr(f, k)) for k in ("delta_p", "delta_q", "delta_v", "linearized_ba", "linearized_bg", "linearized_acc", "linearized_gyr")}
            pre.update(sum_dt=f.sum_dt, jacobian=np.array(f.jacobian).reshape(15, 15))
        return dict(stamp=f.stamp, R=np.array(f.R), T=np.array(f.T), key=bool(f.is_key_frame), samples=n, pre=pre, dt=dt[:n].copy(), acc=acc[:n].copy(),
                    gyr=gyr[:n].copy())

    def last_system(self, which):
        """the normal equations of the last solve -> (A [n, n], b [n], x [n]); which = 0 linear, 1..4 the refinement passes"""
        n = _i32(0)
        self._call("lvi_align_last_system", int(which), C.byref(n), None, None, None, 0)
        Am, b, x = np.zeros((n.value, n.value)), np.zeros(n.value), np.zeros(n.value)
        self._call("lvi_align_last_system", int(which), C.byref(n), _d(Am), _d(b), _d(x), Am.size)
        return Am, b, x

    def key_rotations(self):
        """R of the list's key frames in list order: the kv walk of :457-466"""
        return np.array([f["R"] for f in (self.frame(i) for i in range(len(self))) if f["key"]]).reshape(-1, 9)

    def apply(self, Ps, Rs, x, g, key_R=None):
        """the tail of visualInitialAlign (:450-486) on the host.  Ps [m, 3], Rs [m, 3, 3]: T and R of the window's frames
        (m = frame_count + 1) -> (Ps, Rs, Vs, g, rot_diff, flags)"""
        Ps = np.ascontiguousarray(Ps, np.float64).reshape(-1, 3).copy()
        m = len(Ps)
        Rs = _arr(np.asarray(Rs, np.float64).reshape(-1, 9), (m, 9)).copy()
        key_R = self.key_rotations() if key_R is None else np.ascontiguousarray(key_R, np.float64).reshape(-1, 9)
        x, g = np.ascontiguousarray(x, np.float64).reshape(-1), _arr(g, (3,)).copy()
        Vs, rot, flags = np.zeros((m, 3)), np.zeros(9), _i32(0)
        self.lib.check(self.lib.dll.lvi_align_apply(C.byref(self.params), m - 1, _d(Ps), _d(Rs), _d(Vs), _d(x), len(x), _d(g), _d(key_R) if len(key_R) else None,
                                                    len(key_R), _d(rot), C.byref(flags)), "lvi_align_apply")
        return Ps, Rs.reshape(m, 3, 3), Vs, g, rot.reshape(3, 3), flags.value
