"""Python handle over include/lvi_tbatch.h: up to 8 independent tracker states ("slots") behind one handle, every stage one
launch for all slots.  Mirrors TrackerHotpath's staged method names with per-slot lists; an entry of None means "this slot sits
this call out".  Every slot's results are bit-identical to a TrackerHotpath given the same calls.

The reference compiles NUM_OF_CAM = 1: this is a capability of the library, not a restated reference behaviour.

A separate ABI from include/lvi_hotpath.h: only the product library exports it, so its signature table lives here and is
bound against ``liblvi_hip.so`` alone."""
import ctypes as C

import numpy as np

from . import _abi as A
from .tracker import default_tracker_params

_P = C.POINTER
_vp, _i32, _i64, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double

MAX_BATCH = 8
TBDBG_REDO_MASK = 100

# name -> (restype, argtypes), one entry per function of include/lvi_tbatch.h
TBATCH_SIGNATURES = {
    "lvi_tbatch_abi_version": (_i32, []),
    "lvi_tbatch_create": (_i32, [_P(A.TrackerParams), _i32, _i32, _P(_vp)]),
    "lvi_tbatch_destroy": (None, [_vp]),
    "lvi_tbatch_sync": (_i32, [_vp]),
    "lvi_tbatch_set_equalize": (_i32, [_vp, _i32, _f64, _i32, _i32]),
    "lvi_tbatch_push_images": (_i32, [_vp, _P(_vp), _i32, _i32, _i32]),
    "lvi_tbatch_set_points": (_i32, [_vp, _P(_vp), _P(_i32)]),
    "lvi_tbatch_run_lk": (_i32, [_vp]),
    "lvi_tbatch_get_lk": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _P(_i32)]),
    "lvi_tbatch_set_mask_circles": (_i32, [_vp, _P(_vp), _P(_i32), _i32]),
    "lvi_tbatch_run_gftt_async": (_i32, [_vp, _P(_i32)]),
    "lvi_tbatch_finish_frame": (_i32, [_vp, _P(A.MeiParams), _P(_vp), _P(_i32), _P(_vp), _i32, _P(_i32), _P(_vp)]),
    "lvi_tbatch_debug_get": (_i32, [_vp, _i32, _i32, _vp, _i64, _P(_i64)]),
    "lvi_tbatch_prof_enable": (_i32, [_vp, _i32]),
    "lvi_tbatch_prof_reset": (_i32, [_vp]),
    "lvi_tbatch_prof_read": (_i32, [_vp, _P(A.KernelStat), _i32, _P(_i32)]),
}

_MEI_KEYS = ("xi", "k1", "k2", "p1", "p2", "gamma1", "gamma2", "u0", "v0")


def bind(lib):
    """set the tbatch signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(TBATCH_SIGNATURES)


class TrackerBatch(A.Owned):
    _ptr, _destroy = "_b", "lvi_tbatch_destroy"

    def __init__(self, lib, slots, params=None, device=0, **overrides):
        self.lib = bind(lib)
        self.slots = int(slots)
        self.params = params if params is not None else default_tracker_params(lib, **overrides)
        self._b = C.c_void_p()
        lib.check(lib.dll.lvi_tbatch_create(C.byref(self.params), self.slots, int(device), C.byref(self._b)), "lvi_tbatch_create")

    # ---- per-slot tables ----------------------------------------------------
    def _per_slot(self, items):
        items = list(items)
        if len(items) != self.slots:
            raise ValueError(f"expected {self.slots} per-slot entries, got {len(items)}")
        return items

    def _xy_tables(self, lists):
        """per-slot point lists (None = sits out) -> (kept arrays, pointer table, count table)"""
        arrs = [None if x is None else np.ascontiguousarray(x, np.float32).reshape(-1, 2) for x in self._per_slot(lists)]
        ptrs = (_vp * self.slots)(*[A._ptr(a) if a is not None else None for a in arrs])
        n = (_i32 * self.slots)(*[-1 if a is None else len(a) for a in arrs])
        return arrs, ptrs, n

    def set_equalize(self, on, clip_limit=3.0, tiles=(8, 8)):
        self.lib.check(self.lib.dll.lvi_tbatch_set_equalize(self._b, 1 if on else 0, float(clip_limit), int(tiles[0]), int(tiles[1])), "lvi_tbatch_set_equalize")

    def push_images(self, imgs):
        arrs = [None if x is None else np.ascontiguousarray(x, np.uint8) for x in self._per_slot(imgs)]
        live = [a for a in arrs if a is not None]
        if not live:
            return
        if any(a.ndim != 2 or a.shape != live[0].shape for a in live):
            raise ValueError("all images of one call share their size")
        h, w = live[0].shape
        ptrs = (_vp * self.slots)(*[A._ptr(a) if a is not None else None for a in arrs])
        self.lib.check(self.lib.dll.lvi_tbatch_push_images(self._b, ptrs, w, h, live[0].strides[0]), "lvi_tbatch_push_images")

    def set_points(self, xys):
        arrs, ptrs, n = self._xy_tables(xys)
        self.lib.check(self.lib.dll.lvi_tbatch_set_points(self._b, ptrs, n), "lvi_tbatch_set_points")

    def run_lk(self):
        self.lib.check(self.lib.dll.lvi_tbatch_run_lk(self._b), "lvi_tbatch_run_lk")

    def get_lk(self, slot):
        cap = int(self.params.max_features)
        xy = np.zeros((cap, 2), np.float32)
        st = np.zeros(cap, np.uint8)
        err = np.zeros(cap, np.float32)
        n = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_tbatch_get_lk(self._b, int(slot), A._ptr(xy), A._ptr(st), A._ptr(err), cap, C.byref(n)), "lvi_tbatch_get_lk")
        return xy[:n.value].copy(), st[:n.value].copy(), err[:n.value].copy()

    def set_mask_circles(self, centers, radius):
        arrs, ptrs, n = self._xy_tables(centers)
        self.lib.check(self.lib.dll.lvi_tbatch_set_mask_circles(self._b, ptrs, n, int(radius)), "lvi_tbatch_set_mask_circles")

    def run_gftt_async(self, max_corners):
        mc = (_i32 * self.slots)(*[-1 if m is None else int(m) for m in self._per_slot(max_corners)])
        self.lib.check(self.lib.dll.lvi_tbatch_run_gftt_async(self._b, mc), "lvi_tbatch_run_gftt_async")

    def finish_frame(self, kept, cams=None):
        """per slot: (new corners of a pending run_gftt_async, undistorted [kept ; new] or None); None for a slot that sits out.
        cams: one MEI dict per slot (entries of slots that sit out may be None), or None for no undistortion."""
        arrs, ptrs, nk = self._xy_tables(kept)
        cap = int(self.params.max_features)
        new = [np.zeros((cap, 2), np.float32) for _ in range(self.slots)]
        un = [np.zeros((cap, 2), np.float32) for _ in range(self.slots)]
        n_new = (_i32 * self.slots)(*([0] * self.slots))
        cam_tab = None
        if cams is not None:
            cams = self._per_slot(cams)
            cam_tab = (A.MeiParams * self.slots)(*[A.MeiParams(*[float(c[q]) for q in _MEI_KEYS]) if c is not None else A.MeiParams() for c in cams])
        new_p = (_vp * self.slots)(*[A._ptr(a) for a in new])
        un_p = (_vp * self.slots)(*[A._ptr(a) for a in un])
        self.lib.check(self.lib.dll.lvi_tbatch_finish_frame(self._b, cam_tab, ptrs, nk, new_p, cap, n_new, un_p if cam_tab is not None else None),
                       "lvi_tbatch_finish_frame")
        out = []
        for s in range(self.slots):
            if arrs[s] is None:
                out.append(None)
                continue
            m = n_new[s]
            out.append((new[s][:m].copy(), un[s][:len(arrs[s]) + m].copy() if cam_tab is not None else None))
        return out

    def sync(self):
        self.lib.check(self.lib.dll.lvi_tbatch_sync(self._b), "lvi_tbatch_sync")

    def debug_get(self, slot, what, dtype):
        nb = C.c_int64(0)
        self.lib.check(self.lib.dll.lvi_tbatch_debug_get(self._b, int(slot), int(what), None, 0, C.byref(nb)), "lvi_tbatch_debug_get(size)")
        out = np.zeros(nb.value // np.dtype(dtype).itemsize, dtype)
        if out.size:
            self.lib.check(self.lib.dll.lvi_tbatch_debug_get(self._b, int(slot), int(what), A._ptr(out), out.nbytes, C.byref(nb)), "lvi_tbatch_debug_get")
        return out

    def redo_mask(self):
        """bit s = slot s's GFTT was redone in the radix form during the last finish_frame"""
        return int(self.debug_get(0, TBDBG_REDO_MASK, np.int32)[0])

    def prof_enable(self, on=True):
        self.lib.check(self.lib.dll.lvi_tbatch_prof_enable(self._b, 1 if on else 0), "lvi_tbatch_prof_enable")

    def prof_reset(self):
        self.lib.check(self.lib.dll.lvi_tbatch_prof_reset(self._b), "lvi_tbatch_prof_reset")

    def prof_read(self):
        stats = (A.KernelStat * 128)()
        n = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_tbatch_prof_read(self._b, stats, 128, C.byref(n)), "lvi_tbatch_prof_read")
        return [dict(name=stats[i].name.decode(), launches=stats[i].launches, total_ms=stats[i].total_ms, bytes_alg=stats[i].bytes_alg)
                for i in range(n.value)]
