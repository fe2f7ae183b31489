"""Python handle over include/lvi_fmatb.h: rejectWithF's cv::findFundamentalMat (feature_tracker.cpp:229) for up to
MAX_BATCH independent point-pair sets in one call — one stream, one wait, (active slots) + 1 launches; every slot's
results are bit-identical to a FundamentalRansac given the same inputs.

A separate ABI from include/lvi_fmat.h: only the product library exports it, so its signature table lives here and is
bound against ``liblvi_hip.so`` alone."""
import ctypes as C

import numpy as np

from . import _abi as A
from .fmat import FmatInfo, _info_dict
from .tbatch import MAX_BATCH

_P = C.POINTER
_vp, _i32, _i64, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double

# name -> (restype, argtypes), one entry per function of include/lvi_fmatb.h
FMATB_SIGNATURES = {
    "lvi_fmatb_abi_version": (_i32, []),
    "lvi_fmatb_create": (_i32, [_i32, _i32, _i32, _i32, _P(_vp)]),
    "lvi_fmatb_destroy": (None, [_vp]),
    "lvi_fmatb_set_check_subset": (_i32, [_vp, _i32]),
    "lvi_fmatb_find": (_i32, [_vp, _P(_vp), _P(_vp), _P(_i32), _P(_f64), _f64, _P(_vp), _P(FmatInfo)]),
    "lvi_fmatb_trace": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _P(_i32)]),
    "lvi_fmatb_counters": (_i32, [_vp, _P(_i64), _P(_i64), _P(_i64), _P(_i64)]),
}


def bind(lib):
    """set the fmatb signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(FMATB_SIGNATURES)


class FundamentalRansacBatch(A.Owned):
    """`slots` FundamentalRansac handles behind one call: the sample stream of slot s + 1 is drawn on the host while the
    device scores slot s, then one launch walks all slots and one wait ends the call."""
    _destroy = "lvi_fmatb_destroy"

    def __init__(self, lib, slots, max_points=2048, max_iters=1000, device=0):
        self.lib = bind(lib)
        self.slots = int(slots)
        self.max_points = int(max_points)
        self.max_iters = int(max_iters)
        self._h = C.c_void_p()
        lib.check(lib.dll.lvi_fmatb_create(int(device), self.slots, self.max_points, self.max_iters, C.byref(self._h)), "lvi_fmatb_create")

    def set_check_subset(self, mode):
        """FundamentalRansac.set_check_subset for all slots"""
        self.lib.check(self.lib.dll.lvi_fmatb_set_check_subset(self._h, int(mode)), "lvi_fmatb_set_check_subset")

    def find(self, pairs, thresholds, confidence=0.99):
        """pairs: per slot (pts1 [n, 2], pts2 [n, 2]) or None (the slot sits out); thresholds: one per slot (or one for all)
        -> per slot (status [n] uint8, info dict) or None"""
        if len(pairs) != self.slots:
            raise ValueError("one pair (or None) per slot")
        thr = [float(thresholds)] * self.slots if np.isscalar(thresholds) else [float(t) for t in thresholds]
        if len(thr) != self.slots:
            raise ValueError("one threshold per slot")
        a, b, st = [None] * self.slots, [None] * self.slots, [None] * self.slots
        n = (_i32 * self.slots)(*([-1] * self.slots))
        for s, pr in enumerate(pairs):
            if pr is None:
                continue
            a[s] = np.ascontiguousarray(pr[0], np.float32).reshape(-1, 2)
            b[s] = np.ascontiguousarray(pr[1], np.float32).reshape(-1, 2)
            if len(a[s]) != len(b[s]):
                raise ValueError("pts1 and pts2 differ in length")
            st[s] = np.zeros(max(len(a[s]), 1), np.uint8)
            n[s] = len(a[s])

        def table(arrs):
            return (_vp * self.slots)(*[A._ptr(x) if x is not None else None for x in arrs])
        info = (FmatInfo * self.slots)()
        self.lib.check(self.lib.dll.lvi_fmatb_find(self._h, table(a), table(b), n, (_f64 * self.slots)(*thr), float(confidence), table(st), info),
                       "lvi_fmatb_find")
        return [None if pairs[s] is None else (st[s][:n[s]].copy(), _info_dict(info[s])) for s in range(self.slots)]

    def trace(self, slot):
        """FundamentalRansac.trace of one slot of the last find; a slot that sat out has no hypotheses"""
        m = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_fmatb_trace(self._h, int(slot), None, None, None, None, 0, C.byref(m)), "lvi_fmatb_trace")
        k = max(m.value, 1)
        sub = np.zeros((k, 7), np.int32); nm = np.zeros(k, np.int32); F = np.zeros((k, 3, 3, 3), np.float64); sc = np.zeros((k, 3), np.int32)
        self.lib.check(self.lib.dll.lvi_fmatb_trace(self._h, int(slot), A._ptr(sub), A._ptr(nm), A._ptr(F), A._ptr(sc), m.value, C.byref(m)), "lvi_fmatb_trace")
        n = m.value
        return dict(subsets=sub[:n].copy(), nmodels=nm[:n].copy(), F=F[:n].copy(), score=sc[:n].copy())

    def counters(self):
        """totals since creation: dict(calls, hyp_launches, walk_launches, waits)"""
        v = [_i64(0) for _ in range(4)]
        self.lib.check(self.lib.dll.lvi_fmatb_counters(self._h, *[C.byref(x) for x in v]), "lvi_fmatb_counters")
        return dict(zip(("calls", "hyp_launches", "walk_launches", "waits"), (int(x.value) for x in v)))
