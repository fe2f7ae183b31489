"""Python handle over include/lvi_preint.h: the IMU preintegration of vins_estimator's sliding window (Estimator::processIMU,
estimator.cpp:82-116; IntegrationBase, factor/integration_base.h:9-158; the preintegration side of both slides, :988-1016 and
:1043-1068; the repropagate loop of the lidar initialisation, :215-269) on the GPU — DESIGN §29.

A separate ABI from include/lvi_hotpath.h: only the product library exports it, so its signature table lives here and is
bound against ``liblvi_hip.so`` alone.  The record is the window solve's lvi_win_imu."""
import ctypes as C

import numpy as np

from . import _abi as A
from ._abi import _arr, _d
from .win import IMU_DTYPE

_P = C.POINTER
_vp, _i32, _u32, _f64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_double

SLOTS, MAX_SAMPLES, CHUNK = 11, 8192, 16
WINDOW = SLOTS - 1


class PreintCaps(C.Structure):
    _fields_ = [("max_samples", _i32), ("reserved", _i32)]


class PreintParams(C.Structure):
    _fields_ = [("acc_n", _f64), ("gyr_n", _f64), ("acc_w", _f64), ("gyr_w", _f64), ("G", _f64 * 3)]


class PreintNav(C.Structure):
    _fields_ = [("P", _f64 * 3), ("R", _f64 * 9), ("V", _f64 * 3), ("Ba", _f64 * 3), ("Bg", _f64 * 3)]


# name -> (restype, argtypes), one entry per function of include/lvi_preint.h
PREINT_SIGNATURES = {
    "lvi_preint_abi_version": (_i32, []),
    "lvi_preint_params_default": (None, [_P(PreintParams)]),
    "lvi_preint_create": (_i32, [_i32, _P(PreintCaps), _P(_vp)]),
    "lvi_preint_destroy": (None, [_vp]),
    "lvi_preint_set_params": (_i32, [_vp, _P(PreintParams)]),
    "lvi_preint_clear": (_i32, [_vp]),
    "lvi_preint_set_nav": (_i32, [_vp, _P(PreintNav)]),
    "lvi_preint_get_nav": (_i32, [_vp, _P(PreintNav)]),
    "lvi_preint_push": (_i32, [_vp, _i32, _i32, _P(_f64), _P(_f64), _P(_f64)]),
    "lvi_preint_repropagate": (_i32, [_vp, _u32, _P(_f64), _P(_f64)]),
    "lvi_preint_slide_old": (_i32, [_vp]),
    "lvi_preint_slide_new": (_i32, [_vp]),
    "lvi_preint_get": (_i32, [_vp, _i32, _vp, _P(_i32)]),
    "lvi_preint_get_samples": (_i32, [_vp, _i32, _i32, _P(_i32), _P(_f64), _P(_f64), _P(_f64)]),
    "lvi_preint_evaluate": (_i32, [_vp, _i32, _P(_f64), _P(_f64), _P(_f64), _P(_f64), _P(_f64), _P(_f64)]),
}


def bind(lib):
    """set the preintegration signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(PREINT_SIGNATURES)


class ImuWindow(A.Owned):
    """pre_integrations[0..WINDOW_SIZE], the newest slot's navigation state and the estimator's acc_0 / gyr_0 / first_imu,
    resident on the device.  process_imu buffers on the host and flush pushes the buffer as one call: the per-image cadence
    of the estimator node."""
    _destroy = "lvi_preint_destroy"
    imu_dtype = IMU_DTYPE

    def __init__(self, lib, device=0, max_samples=2048, **params):
        self.lib = bind(lib)
        self.caps = PreintCaps(int(max_samples), 0)
        self._h = C.c_void_p()
        self._buf = []
        lib.check(lib.dll.lvi_preint_create(int(device), C.byref(self.caps), C.byref(self._h)), "lvi_preint_create")
        self.params = PreintParams()
        lib.dll.lvi_preint_params_default(C.byref(self.params))
        if params:
            self.set_params(**params)

    def _call(self, name, *args):
        return self.lib.check(getattr(self.lib.dll, name)(self._h, *args), name)

    def set_params(self, **kw):
        """acc_n, gyr_n, acc_w, gyr_w, G (three values)"""
        p = PreintParams.from_buffer_copy(self.params)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(f"lvi_preint_params has no field {k}")
            setattr(p, k, (_f64 * 3)(*v) if k == "G" else v)
        self._call("lvi_preint_set_params", C.byref(p))
        self.params = p

    def clear(self):
        """clearState"""
        self._buf = []
        self._call("lvi_preint_clear")

    # ---- the samples
    def process_imu(self, dt, acc, gyr):
        """processIMU: buffered on the host until flush"""
        self._buf.append((float(dt), *(float(v) for v in acc), *(float(v) for v in gyr)))

    def flush(self, frame_count):
        """the buffered samples as one push with this frame_count"""
        b = np.array(self._buf, np.float64).reshape(-1, 7)
        self.push(frame_count, b[:, 0], b[:, 1:4], b[:, 4:7])
        self._buf = []

    def push(self, frame_count, dt, acc, gyr):
        dt = np.ascontiguousarray(dt, np.float64).reshape(-1)
        acc, gyr = _arr(np.asarray(acc, np.float64).reshape(-1, 3), (len(dt), 3)), _arr(np.asarray(gyr, np.float64).reshape(-1, 3), (len(dt), 3))
        self._call("lvi_preint_push", int(frame_count), len(dt), _d(dt), _d(acc), _d(gyr))

    # ---- the navigation state
    def set_nav(self, P, R, V, Ba, Bg):
        """Ps / Rs / Vs / Bas / Bgs of the newest slot: after every solve, before the slide"""
        n = PreintNav()
        for k, v, shape in (("P", P, (3,)), ("R", R, (3, 3)), ("V", V, (3,)), ("Ba", Ba, (3,)), ("Bg", Bg, (3,))):
            a = _arr(v, shape).reshape(-1)
            setattr(n, k, (_f64 * len(a))(*a))
        self._call("lvi_preint_set_nav", C.byref(n))

    def nav(self):
        """-> dict(P [3], R [3, 3], V [3], Ba [3], Bg [3])"""
        n = PreintNav()
        self._call("lvi_preint_get_nav", C.byref(n))
        return dict(P=np.array(n.P), R=np.array(n.R).reshape(3, 3), V=np.array(n.V), Ba=np.array(n.Ba), Bg=np.array(n.Bg))

    # ---- the slots
    def count(self, slot):
        n = _i32(0)
        self._call("lvi_preint_get", int(slot), None, C.byref(n))
        return n.value

    def _samples_or_zero(self, slot):
        """the slot's sample count, 0 for a slot that does not exist"""
        n = _i32(0)
        st = self.lib.dll.lvi_preint_get(self._h, int(slot), None, C.byref(n))
        if st == A.LVI_ERR_STATE:
            return 0
        self.lib.check(st, "lvi_preint_get")
        return n.value

    def record(self, slot):
        """-> a one-element win.IMU_DTYPE array with ids 0: what WindowSolver.add_imu and VinsWindowOptimizer.set_imu take"""
        r = np.zeros(1, IMU_DTYPE)
        self._call("lvi_preint_get", int(slot), r.ctypes.data_as(_vp), None)
        return r

    def samples(self, slot):
        """-> (dt [n], acc [n, 3], gyr [n, 3])"""
        n = self.count(slot)
        dt, acc, gyr = np.zeros(max(1, n)), np.zeros((max(1, n), 3)), np.zeros((max(1, n), 3))
        self._call("lvi_preint_get_samples", int(slot), len(dt), None, _d(dt), _d(acc), _d(gyr))
        return dt[:n].copy(), acc[:n].copy(), gyr[:n].copy()

    def repropagate(self, Bas, Bgs, slots=None):
        """IntegrationBase::repropagate of the named slots (all eleven by default) with Bas [11, 3], Bgs [11, 3]: one launch"""
        Bas, Bgs = _arr(Bas, (SLOTS, 3)), _arr(Bgs, (SLOTS, 3))
        mask = 0
        for i in (range(SLOTS) if slots is None else slots):
            if not 0 <= int(i) < SLOTS:
                raise ValueError(f"slot {i} is outside 0..{WINDOW}")
            mask |= 1 << int(i)
        self._call("lvi_preint_repropagate", mask, _d(Bas), _d(Bgs))

    def slide_old(self):
        self._call("lvi_preint_slide_old")

    def slide_new(self):
        self._call("lvi_preint_slide_new")

    def evaluate(self, slot, pose_i, sb_i, pose_j, sb_j):
        """IMUFactor::Evaluate of the slot's record -> (residual [15], [J 15x7, J 15x9, J 15x7, J 15x9])"""
        a, b, c, d = _arr(pose_i, (7,)), _arr(sb_i, (9,)), _arr(pose_j, (7,)), _arr(sb_j, (9,))
        r, J = np.zeros(15), np.zeros(15 * 32)
        self._call("lvi_preint_evaluate", int(slot), _d(a), _d(b), _d(c), _d(d), _d(r), _d(J))
        return r, [J[0:105].reshape(15, 7).copy(), J[105:240].reshape(15, 9).copy(), J[240:345].reshape(15, 7).copy(), J[345:480].reshape(15, 9).copy()]

    # ---- towards the solve and the marginalisation
    def fill(self, optimizer):
        """pre_integrations[1..WINDOW_SIZE] of a host_api.VinsWindowOptimizer; a slot without samples, or one that does not
        exist yet, gives no factor (the optimiser applies the sum_dt > 10 skip of estimator.cpp:740 itself)"""
        for j in range(1, SLOTS):
            optimizer.set_imu(j, self.record(j) if self._samples_or_zero(j) > 0 else None)

    def fill_marginalizer(self, marginalizer, poses, speed_biases):
        """the IMU block of MARGIN_OLD (estimator.cpp:837-844): pre_integrations[1] evaluated at blocks 0 and 1"""
        poses, sbs = np.asarray(poses, np.float64), np.asarray(speed_biases, np.float64)
        if self._samples_or_zero(1) == 0:
            return marginalizer.set_imu(0.0)
        r, J = self.evaluate(1, poses[0], sbs[0], poses[1], sbs[1])
        return marginalizer.set_imu(float(self.record(1)["sum_dt"][0]), r, J)

    def lidar_initialise(self, feature_manager, frames, ric=None):
        """The lidar branch of Estimator::initialStructure (estimator.cpp:215-269).  frames: eleven dicts of reset_id, T, R, V,
        Ba, Bg, gravity.  -> None when a reset_id is negative or differs from frame 0's (nothing changes), else
        (Ps [11, 3], Rs [11, 3, 3], Vs [11, 3], Bas [11, 3], Bgs [11, 3], g [3]) after every slot was repropagated with the
        frames' biases, the handle's G set to g = (0, 0, gravity of frame 0) as :253 sets the estimator's, every depth
        cleared to -1 and the table triangulated with tic = 0 and ric (RIC[0], the identity by default).  feature_manager: a fman.FeatureTable.  The SFM path the reference falls back to is not restated."""
        if len(frames) != SLOTS:
            raise ValueError(f"expected {SLOTS} frames")
        if any(f["reset_id"] < 0 or f["reset_id"] != frames[0]["reset_id"] for f in frames):
            return None
        Ps, Rs, Vs = (np.array([np.asarray(f[k], np.float64) for f in frames]) for k in ("T", "R", "V"))
        Bas, Bgs = (np.array([np.asarray(f[k], np.float64) for f in frames]) for k in ("Ba", "Bg"))
        self.repropagate(Bas, Bgs)
        g = np.array([0.0, 0.0, float(frames[0]["gravity"])])
        self.set_params(G=g)                                 # :253: every later navigation step and IMUFactor reads the new g
        n = len(feature_manager.depth_vector())
        feature_manager.clear_depth(np.full(n, -1.0))
        feature_manager.triangulate(Ps, Rs, np.zeros(3), np.eye(3) if ric is None else np.asarray(ric, np.float64))
        return Ps, Rs, Vs, Bas, Bgs, g
