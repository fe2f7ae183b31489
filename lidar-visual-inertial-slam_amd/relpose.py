"""Python handle over include/lvi_relpose.h: the initial two-view pose of vins_estimator's visual initialisation
(MotionEstimator::solveRelativeRT, initial/solve_5pts.cpp:193-227; Estimator::relativePose, estimator.cpp:493-522) on the GPU
— a restatement of OpenCV 4.5.x recoverPose, DESIGN §30.

A separate ABI from include/lvi_hotpath.h: only the product library exports it, so its signature table lives here and is
bound against ``liblvi_hip.so`` alone."""
import ctypes as C

import numpy as np

from . import _abi as A
from ._abi import _d
from . import fmat as _fmat
from .fmat import FmatInfo

_P = C.POINTER
_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double

MIN_POINTS, MIN_INLIERS, CHUNK = 15, 12, 64
MAX_POINTS = 3072                      # LVI_FMAT_MAX_POINTS
DEGENERATE, NO_MODEL, TOO_FEW = 1, 2, 4
WINDOW = 10                            # WINDOW_SIZE
MIN_PAIRS, FOCAL_LENGTH, MIN_PARALLAX_PX = 20, 460, 30        # estimator.cpp:500, :513


class RelposeParams(C.Structure):
    _fields_ = [("threshold", _f64), ("confidence", _f64), ("distance_thresh", _f64)]


class RelposePose(C.Structure):
    _fields_ = [("R", _f64 * 9), ("t", _f64 * 3), ("sv", _f64 * 3), ("good", _i32 * 4), ("chosen", _i32), ("n_inliers", _i32), ("flags", _i32),
                ("sweeps", _i32)]


class RelposeResult(C.Structure):
    _fields_ = [("Rotation", _f64 * 9), ("Translation", _f64 * 3), ("average_parallax", _f64), ("ok", _i32), ("flags", _i32), ("pose", RelposePose),
                ("info", FmatInfo)]


# name -> (restype, argtypes), one entry per function of include/lvi_relpose.h
RELPOSE_SIGNATURES = {
    "lvi_relpose_abi_version": (_i32, []),
    "lvi_relpose_params_default": (None, [_P(RelposeParams)]),
    "lvi_relpose_create": (_i32, [_i32, _i32, _i32, _P(_vp)]),
    "lvi_relpose_destroy": (None, [_vp]),
    "lvi_relpose_set_params": (_i32, [_vp, _P(RelposeParams)]),
    "lvi_relpose_recover": (_i32, [_vp, _P(_f64), _vp, _vp, _i32, _vp, _f64, _P(RelposePose)]),
    "lvi_relpose_solve": (_i32, [_vp, _P(_f64), _i32, _P(RelposeResult), _vp]),
    "lvi_relpose_average_parallax": (_f64, [_P(_f64), _i32]),
    "lvi_relpose_last": (_i32, [_vp, _P(_f64), _vp, _i32, _P(_i32)]),
    "lvi_relpose_fmat": (_vp, [_vp]),
}


def bind(lib):
    """set the two-view signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    _fmat.bind(lib)
    return lib.bind(RELPOSE_SIGNATURES)


def _pose_dict(p):
    return dict(R=np.array(p.R).reshape(3, 3), t=np.array(p.t), sv=np.array(p.sv), good=list(p.good), chosen=p.chosen, n_inliers=p.n_inliers, flags=p.flags,
                sweeps=p.sweeps)


class _BorrowedFmat(_fmat.FundamentalRansac):
    """the lvi_fmat a RelativePose owns, for trace(): never destroyed from here"""
    _own = False

    def __init__(self, lib, handle, max_points, max_iters):
        self.lib, self.max_points, self.max_iters, self._h = lib, max_points, max_iters, C.c_void_p(handle)


class RelativePose(A.Owned):
    """m_estimator and the loop of Estimator::relativePose.  One handle serves calls of up to max_points correspondences."""
    _destroy = "lvi_relpose_destroy"

    def __init__(self, lib, device=0, max_points=1024, max_iters=1000, **params):
        self.lib = bind(lib)
        self.max_points, self.max_iters = int(max_points), int(max_iters)
        self._h = C.c_void_p()
        lib.check(lib.dll.lvi_relpose_create(int(device), self.max_points, self.max_iters, C.byref(self._h)), "lvi_relpose_create")
        self.params = RelposeParams()
        lib.dll.lvi_relpose_params_default(C.byref(self.params))
        if params:
            self.set_params(**params)

    def _call(self, name, *args):
        return self.lib.check(getattr(self.lib.dll, name)(self._h, *args), name)

    def set_params(self, **kw):
        """threshold, confidence, distance_thresh"""
        p = RelposeParams.from_buffer_copy(self.params)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(f"lvi_relpose_params has no field {k}")
            setattr(p, k, v)
        self._call("lvi_relpose_set_params", C.byref(p))
        self.params = p

    def fmat(self):
        """a view of the owned FundamentalRansac (its trace() describes the last solve)"""
        return _BorrowedFmat(self.lib, self.lib.dll.lvi_relpose_fmat(self._h), self.max_points, self.max_iters)

    def recover(self, E, pts1, pts2, mask=None, distance_thresh=50.0):
        """cv::recoverPose with the identity camera matrix: E [3, 3], pts1, pts2 [n, 2] (f32), mask [n] or None ->
        dict(R, t, sv, good [4], chosen, n_inliers, flags, sweeps, mask [n] uint8: the chosen candidate's)"""
        E = np.ascontiguousarray(E, np.float64).reshape(-1)
        if E.shape != (9,):
            raise ValueError("E must have nine entries")
        a = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
        if len(a) != len(b):
            raise ValueError("pts1 and pts2 differ in length")
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8).reshape(-1).copy()
            if len(m) != len(a):
                raise ValueError("the mask and the points differ in length")
        p = RelposePose()
        self._call("lvi_relpose_recover", _d(E), A._ptr(a), A._ptr(b), len(a), A._ptr(m) if m is not None and len(m) else None, float(distance_thresh),
                   C.byref(p))
        out = _pose_dict(p)
        out["mask"] = m if m is not None else self.last()[1][p.chosen]
        return out

    def last(self):
        """the last recover -> (cand [4] of (R [3, 3], t [3]), masks [4, n] uint8)"""
        n = _i32(0)
        self._call("lvi_relpose_last", None, None, 0, C.byref(n))
        cand, masks = np.zeros((4, 12)), np.zeros((4, max(1, n.value)), np.uint8)
        self._call("lvi_relpose_last", _d(cand), A._ptr(masks), masks.shape[1], None)
        return [(cand[c, :9].reshape(3, 3).copy(), cand[c, 9:].copy()) for c in range(4)], masks[:, :n.value].copy()

    def solve(self, pairs):
        """solveRelativeRT on one getCorresponding result, pairs [n, 2, 3] or [n, 6] -> dict(ok, Rotation, Translation,
        average_parallax, flags, pose, info, status [n] uint8)"""
        pairs = np.ascontiguousarray(pairs, np.float64).reshape(-1, 6)
        r, st = RelposeResult(), np.zeros(max(1, len(pairs)), np.uint8)
        self._call("lvi_relpose_solve", _d(pairs), len(pairs), C.byref(r), A._ptr(st))
        return dict(ok=bool(r.ok), Rotation=np.array(r.Rotation).reshape(3, 3), Translation=np.array(r.Translation), average_parallax=r.average_parallax,
                    flags=r.flags, pose=_pose_dict(r.pose), info=_fmat._info_dict(r.info), status=st[:len(pairs)].copy())

    def average_parallax(self, pairs):
        """the gate's average parallax of estimator.cpp:502-512, in normalised units"""
        pairs = np.ascontiguousarray(pairs, np.float64).reshape(-1, 6)
        return float(self.lib.dll.lvi_relpose_average_parallax(_d(pairs), len(pairs)))

    def find(self, feature_table):
        """Estimator::relativePose over a fman.FeatureTable (anything with corresponding(l, r)) -> (ok, l, R, T, records): the
        first frame i of 0..WINDOW_SIZE-1 with more than 20 pairs to the newest frame, an average parallax above 30 pixels
        and a solve that succeeds.  records: one dict per frame visited (frame, n, average_parallax, and the solve's result
        when it ran).  As in the reference a failed solve has still overwritten R and T; only ok says whether they mean
        anything."""
        R, T, records = np.eye(3), np.zeros(3), []
        for i in range(WINDOW):
            pairs = np.asarray(feature_table.corresponding(i, WINDOW), np.float64).reshape(-1, 6)
            rec = dict(frame=i, n=len(pairs), average_parallax=None, solved=False, ok=False)
            records.append(rec)
            if len(pairs) > MIN_PAIRS:
                rec["average_parallax"] = self.average_parallax(pairs)
                if rec["average_parallax"] * FOCAL_LENGTH > MIN_PARALLAX_PX:
                    s = self.solve(pairs)
                    rec.update(solved=True, ok=s["ok"], result=s)
                    R, T = s["Rotation"], s["Translation"]
                    if s["ok"]:
                        return True, i, R, T, records
        return False, -1, R, T, records
