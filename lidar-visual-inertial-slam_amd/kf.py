"""Python handle over include/lvi_kf.h: pose_graph keyframes on the GPU — the image work of the KeyFrame constructor
(pose_graph/src/keyframe.cpp:14-73: blur, FAST, BRIEF, MEI lift) and findConnection's descriptor search (:81-131,
266-271) — a restatement of OpenCV 4.5.x and DVision, DESIGN §14.

A separate ABI from include/lvi_hotpath.h: only the product library exports it, so its signature table lives here and
is bound against ``liblvi_hip.so`` alone."""
import ctypes as C

import numpy as np

from . import _abi as A

_P = C.POINTER
_vp, _i32 = C.c_void_p, C.c_int32

KF_TRUNCATED = 16
PAIRS = 256


class KfInfo(C.Structure):
    _fields_ = [("n_keypoints_found", C.c_int32), ("n_keypoints_stored", C.c_int32), ("n_window", C.c_int32), ("reserved", C.c_int32)]


# name -> (restype, argtypes), one entry per function of include/lvi_kf.h
KF_SIGNATURES = {
    "lvi_kf_abi_version": (_i32, []),
    "lvi_kf_create": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _P(_i32), _P(_i32), _P(_i32), _P(_i32), _P(_vp)]),
    "lvi_kf_destroy": (None, [_vp]),
    "lvi_kf_describe": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _i32, _P(A.MeiParams), _P(KfInfo)]),
    "lvi_kf_get": (_i32, [_vp, _i32, _P(_i32), _vp, _vp, _vp, _vp, _vp]),
    "lvi_kf_put": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "lvi_kf_release": (_i32, [_vp, _i32]),
    "lvi_kf_match": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp]),
    "lvi_kf_debug_maps": (_i32, [_vp, _vp, _vp, _P(_i32)]),
}


def bind(lib):
    """set the keyframe signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(KF_SIGNATURES)


def mei_params(cam):
    """dict(xi, k1, k2, p1, p2, gamma1, gamma2, u0, v0) (config.load_camera_yaml's) -> lvi_mei_params, None -> None"""
    if cam is None or isinstance(cam, A.MeiParams):
        return cam
    return A.MeiParams(*[float(cam[k]) for k in ("xi", "k1", "k2", "p1", "p2", "gamma1", "gamma2", "u0", "v0")])


class KeyframeDescriber(A.Owned):
    """The keyframe store of a pose graph on one GPU.  pattern = (x1, y1, x2, y2) of config.load_brief_pattern.  A slot
    holds one keyframe: FAST keypoints (pixel, normalised, descriptors) and window points (pixel, descriptors)."""
    _destroy = "lvi_kf_destroy"

    def __init__(self, lib, pattern, device=0, max_width=1024, max_height=576, max_keypoints=8192, max_window=1024, max_keyframes=16):
        self.lib = bind(lib)
        self.max_width, self.max_height = int(max_width), int(max_height)
        self.max_keypoints, self.max_window, self.max_keyframes = int(max_keypoints), int(max_window), int(max_keyframes)
        pat = [np.ascontiguousarray(p, np.int32).reshape(-1) for p in pattern]
        if len(pat) != 4 or any(len(p) != PAIRS for p in pat):
            raise ValueError("the BRIEF pattern is four arrays of 256 ints")
        self._h = C.c_void_p()
        lib.check(lib.dll.lvi_kf_create(int(device), self.max_width, self.max_height, self.max_keypoints, self.max_window, self.max_keyframes,
                                        *[p.ctypes.data_as(_P(_i32)) for p in pat], C.byref(self._h)), "lvi_kf_create")

    def describe(self, slot, img, window_xy=None, cam=None):
        """the KeyFrame constructor's image work into `slot`; img = a 2-D uint8 array (a view with a row stride is read in
        place), window_xy [n, 2] = point_2d_uv -> dict(n_keypoints_found, n_keypoints_stored, n_window, truncated)"""
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError("img must be a 2-D uint8 array")
        if img.strides[1] != 1 or img.strides[0] < img.shape[1]:
            img = np.ascontiguousarray(img)
        win = np.ascontiguousarray(window_xy if window_xy is not None else np.zeros((0, 2)), np.float32).reshape(-1, 2)
        info = KfInfo()
        c = mei_params(cam)
        st = self.lib.check(self.lib.dll.lvi_kf_describe(self._h, int(slot), C.c_void_p(img.ctypes.data), img.shape[1], img.shape[0], img.strides[0],
                                                         A._ptr(win) if len(win) else None, len(win), C.byref(c) if c is not None else None,
                                                         C.byref(info)), "lvi_kf_describe")
        return dict(n_keypoints_found=info.n_keypoints_found, n_keypoints_stored=info.n_keypoints_stored, n_window=info.n_window,
                    truncated=st == KF_TRUNCATED)

    def get(self, slot):
        """dict(keypoints [k, 2] f32, keypoints_norm [k, 2] f32, kp_desc [k, 4] u64, window_xy [n, 2] f32, win_desc [n, 4] u64)"""
        cnt = (C.c_int32 * 2)()
        self.lib.check(self.lib.dll.lvi_kf_get(self._h, int(slot), cnt, None, None, None, None, None), "lvi_kf_get")
        k, n = cnt[0], cnt[1]
        kp = np.zeros((max(k, 1), 2), np.float32); kn = np.zeros((max(k, 1), 2), np.float32); kd = np.zeros((max(k, 1), 4), np.uint64)
        wx = np.zeros((max(n, 1), 2), np.float32); wd = np.zeros((max(n, 1), 4), np.uint64)
        self.lib.check(self.lib.dll.lvi_kf_get(self._h, int(slot), cnt, A._ptr(kp), A._ptr(kn), A._ptr(kd), A._ptr(wx), A._ptr(wd)), "lvi_kf_get")
        return dict(keypoints=kp[:k].copy(), keypoints_norm=kn[:k].copy(), kp_desc=kd[:k].copy(), window_xy=wx[:n].copy(), win_desc=wd[:n].copy())

    def put(self, slot, keypoints=None, keypoints_norm=None, kp_desc=None, window_xy=None, win_desc=None):
        """upload a keyframe (the loadKeyFrame constructor); the counts come from kp_desc and win_desc, a missing array of a
        present group stores zeros"""
        def arr(a, dt, width):
            return None if a is None else np.ascontiguousarray(a, dt).reshape(-1, width)
        kp, kn, kd = arr(keypoints, np.float32, 2), arr(keypoints_norm, np.float32, 2), arr(kp_desc, np.uint64, 4)
        wx, wd = arr(window_xy, np.float32, 2), arr(win_desc, np.uint64, 4)
        k = max([len(a) for a in (kp, kn, kd) if a is not None], default=0)
        n = max([len(a) for a in (wx, wd) if a is not None], default=0)
        if any(a is not None and len(a) != k for a in (kp, kn, kd)) or any(a is not None and len(a) != n for a in (wx, wd)):
            raise ValueError("arrays of one group differ in length")
        p = lambda a: A._ptr(a) if a is not None and len(a) else None  # noqa: E731
        self.lib.check(self.lib.dll.lvi_kf_put(self._h, int(slot), k, p(kp), p(kn), p(kd), n, p(wx), p(wd)), "lvi_kf_put")

    def release(self, slot):
        self.lib.check(self.lib.dll.lvi_kf_release(self._h, int(slot)), "lvi_kf_release")

    def match(self, cur_slot, old_slot):
        """searchByBRIEFDes: cur's window descriptors against old's keypoint descriptors -> (status u8 [n], index i32 [n]
        (-1 = no distance below 128), dist i32 [n])"""
        cnt = (C.c_int32 * 2)()
        self.lib.check(self.lib.dll.lvi_kf_get(self._h, int(cur_slot), cnt, None, None, None, None, None), "lvi_kf_get")
        n = cnt[1]
        st = np.zeros(max(n, 1), np.uint8); ix = np.full(max(n, 1), -1, np.int32); ds = np.zeros(max(n, 1), np.int32)
        self.lib.check(self.lib.dll.lvi_kf_match(self._h, int(cur_slot), int(old_slot), A._ptr(st), A._ptr(ix), A._ptr(ds)), "lvi_kf_match")
        return st[:n].copy(), ix[:n].copy(), ds[:n].copy()

    def debug_maps(self):
        """(blurred image, FAST score map) of the last describe, uint8 [h, w]"""
        wh = (C.c_int32 * 2)()
        self.lib.check(self.lib.dll.lvi_kf_debug_maps(self._h, None, None, wh), "lvi_kf_debug_maps")
        bl = np.zeros((wh[1], wh[0]), np.uint8); sc = np.zeros((wh[1], wh[0]), np.uint8)
        self.lib.check(self.lib.dll.lvi_kf_debug_maps(self._h, A._ptr(bl), A._ptr(sc), wh), "lvi_kf_debug_maps")
        return bl, sc
