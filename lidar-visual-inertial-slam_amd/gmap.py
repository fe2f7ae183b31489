"""Python handle over include/lvi_gmap.h: mapOptimization's global map (publishGlobalMap's and save_map's fuse of the
keyframe clouds + VoxelGrid, mapOptimization.cpp:179-236 and :460-510) over the device keyframe store of a lidar handle.

A separate ABI from include/lvi_hotpath.h: only the product library exports it, so its signature table lives here and
is bound against ``liblvi_hip.so`` alone."""
import ctypes as C

import numpy as np

from . import _abi as A

_P = C.POINTER
_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

CORNER, SURF, CORNER_SURF = 0, 1, 2
FUSED, FILTERED = 0, 1
MAX_POINTS = 1 << 25


class GmapInfo(C.Structure):
    _fields_ = [("n_fused", _i32), ("n_out", _i32), ("overflow", _i32), ("filtered", _i32)]


# name -> (restype, argtypes), one entry per function of include/lvi_gmap.h
GMAP_SIGNATURES = {
    "lvi_gmap_abi_version": (_i32, []),
    "lvi_gmap_reserve": (_i32, [_vp, _i32]),
    "lvi_gmap_release": (_i32, [_vp]),
    "lvi_gmap_arena_bytes": (_i32, [_vp, _P(_i64)]),
    "lvi_gmap_build": (_i32, [_vp, _P(_i32), _i32, _i32, _f32, _P(_i32)]),
    "lvi_gmap_result": (_i32, [_vp, _P(GmapInfo)]),
    "lvi_gmap_fetch": (_i32, [_vp, _i32, _i32, _i32, _vp]),
    "lvi_gmap_debug_voxel": (_i32, [_vp, _vp, _vp, _i32, _P(_i32)]),
}


def bind(lib):
    """set the global-map signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(GMAP_SIGNATURES)


class GlobalMap:
    """the global-map calls of one lidar handle (a LidarHotpath, or the handle a SequentialMapper owns).  result() and
    fetch() may run on another thread while the owner runs scans; build / reserve / release may not (include/lvi_gmap.h)."""

    def __init__(self, lidar_handle):
        self.lib = bind(lidar_handle.lib)
        self.lidar = lidar_handle
        self._h = lidar_handle._h

    def reserve(self, max_points):
        self.lib.check(self.lib.dll.lvi_gmap_reserve(self._h, int(max_points)), "lvi_gmap_reserve")

    def release(self):
        self.lib.check(self.lib.dll.lvi_gmap_release(self._h), "lvi_gmap_release")

    def arena_bytes(self):
        b = _i64(0)
        self.lib.check(self.lib.dll.lvi_gmap_arena_bytes(self._h, C.byref(b)), "lvi_gmap_arena_bytes")
        return b.value

    def build(self, keys, which=CORNER_SURF, leaf=0.0):
        """enqueue the fuse (+ VoxelGrid when leaf > 0); returns the fused size without waiting for the GPU"""
        k = np.ascontiguousarray(keys, np.int32).reshape(-1)
        n = _i32(0)
        self.lib.check(self.lib.dll.lvi_gmap_build(self._h, k.ctypes.data_as(_P(_i32)), len(k), int(which), float(leaf), C.byref(n)),
                       "lvi_gmap_build")
        return n.value

    def result(self):
        r = GmapInfo()
        self.lib.check(self.lib.dll.lvi_gmap_result(self._h, C.byref(r)), "lvi_gmap_result")
        return dict(n_fused=r.n_fused, n_out=r.n_out, overflow=bool(r.overflow), filtered=bool(r.filtered))

    def fetch(self, what=FILTERED, first=0, count=None):
        """points [first, first + count) of the fused or filtered cloud of the last build (count None: to the end)"""
        if count is None:
            r = self.result()
            count = (r["n_fused"] if what == FUSED else r["n_out"]) - int(first)
        out = np.zeros(max(int(count), 1), A.PT_DTYPE)
        self.lib.check(self.lib.dll.lvi_gmap_fetch(self._h, int(what), int(first), int(count), A._ptr(out)), "lvi_gmap_fetch")
        return out[:int(count)]

    def debug_voxel(self):
        """the last build's VoxelGrid: PCL's linear voxel idx in output order and points per voxel"""
        n = _i32(0)
        self.lib.check(self.lib.dll.lvi_gmap_debug_voxel(self._h, None, None, 0, C.byref(n)), "lvi_gmap_debug_voxel")
        cells = np.zeros(max(n.value, 1), np.int32); counts = np.zeros(max(n.value, 1), np.int32)
        self.lib.check(self.lib.dll.lvi_gmap_debug_voxel(self._h, A._ptr(cells), A._ptr(counts), n.value, C.byref(n)), "lvi_gmap_debug_voxel")
        return cells[:n.value].copy(), counts[:n.value].copy()
