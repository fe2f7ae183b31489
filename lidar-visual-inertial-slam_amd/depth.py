"""Python handle over include/lvi_depth.h: the feature tracker's LiDAR depth association (lidar_callback of
feature_tracker_node.cpp:273-377 and DepthRegister::get_depth of feature_tracker.h:116-331) on the GPU.

A separate ABI from include/lvi_hotpath.h: only the product library exports it, so its signature table lives here and
is bound against ``liblvi_hip.so`` alone."""
import ctypes as C

import numpy as np

from . import _abi as A

_P = C.POINTER
_vp, _i32, _f32, _f64 = C.c_void_p, C.c_int32, C.c_float, C.c_double

NUM_BINS = 360

# name -> (restype, argtypes), one entry per function of include/lvi_depth.h
DEPTH_SIGNATURES = {
    "lvi_depth_abi_version": (_i32, []),
    "lvi_depth_create": (_i32, [_i32, _i32, _i32, _i32, _i32, _f64, _P(_vp)]),
    "lvi_depth_destroy": (None, [_vp]),
    "lvi_depth_lidar_cloud": (_i32, [_vp, _vp, _i32, _P(_f32), _f64, _P(_i32)]),
    "lvi_depth_lidar_cloud_device": (_i32, [_vp, _vp, _i32, _P(_f32), _f64, _P(_i32)]),
    "lvi_depth_get": (_i32, [_vp, _P(_f32), _vp, _i32, _vp]),
    "lvi_depth_state": (_i32, [_vp, _P(_i32)]),
    "lvi_depth_set_cloud": (_i32, [_vp, _vp, _i32]),
    "lvi_depth_get_cloud": (_i32, [_vp, _vp, _i32, _P(_i32)]),
    "lvi_depth_debug_voxel": (_i32, [_vp, _vp, _vp, _i32, _P(_i32)]),
    "lvi_depth_debug_range": (_i32, [_vp, _vp]),
    "lvi_depth_debug_sphere": (_i32, [_vp, _vp, _i32, _P(_i32)]),
    "lvi_depth_debug_neighbors": (_i32, [_vp, _vp, _vp, _i32, _P(_i32)]),
    "lvi_depth_set_full_search": (_i32, [_vp, _i32]),
}


def bind(lib):
    """set the depth signatures on a loaded product Library (idempotent); raises AttributeError on a missing export"""
    return lib.bind(DEPTH_SIGNATURES)


def _pose(pose6):
    if pose6 is None:
        return None
    return (C.c_float * 6)(*[float(v) for v in np.asarray(pose6, np.float32).reshape(6)])


class DepthRegister(A.Owned):
    """DepthRegister + the node's lidar window.  pose6 = (x, y, z, roll, pitch, yaw) of the body in the world frame, or
    None when no transform is available."""
    _destroy = "lvi_depth_destroy"

    def __init__(self, lib, device=0, max_clouds=64, max_cloud_points=131072, max_features=150, lidar_skip=3, window_s=5.0):
        self.lib = bind(lib)
        self.max_features = int(max_features)
        self.max_cloud_points = int(max_cloud_points)
        self.max_clouds = int(max_clouds)
        self._h = C.c_void_p()
        lib.check(lib.dll.lvi_depth_create(int(device), int(max_clouds), int(max_cloud_points), int(max_features), int(lidar_skip),
                                           float(window_s), C.byref(self._h)), "lvi_depth_create")

    def lidar_callback(self, cloud, pose6, stamp):
        """one incoming cloud (sensor frame); returns True when it entered the window"""
        pts = A.as_pts(cloud)
        used = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_depth_lidar_cloud(self._h, A._ptr(pts), len(pts), _pose(pose6), float(stamp), C.byref(used)),
                       "lvi_depth_lidar_cloud")
        return bool(used.value)

    def lidar_callback_device(self, d_ptr, n, pose6, stamp):
        used = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_depth_lidar_cloud_device(self._h, C.c_void_p(int(d_ptr)), int(n), _pose(pose6), float(stamp), C.byref(used)),
                       "lvi_depth_lidar_cloud_device")
        return bool(used.value)

    def get_depth(self, pose6, features_xyz):
        """features_xyz [n, 3] = the published points (un_x, un_y, 1) -> the depth channel [n] (> 3.0, else -1)"""
        f = np.ascontiguousarray(features_xyz, np.float32).reshape(-1, 3)
        out = np.full(max(len(f), 1), -1.0, np.float32)
        self.lib.check(self.lib.dll.lvi_depth_get(self._h, _pose(pose6), A._ptr(f), len(f), A._ptr(out)), "lvi_depth_get")
        return out[:len(f)].copy()

    # ---- state and debug views ------------------------------------------------------------------------
    def state(self):
        s = (C.c_int32 * 4)()
        self.lib.check(self.lib.dll.lvi_depth_state(self._h, s), "lvi_depth_state")
        return dict(n_clouds=s[0], lidar_count=s[1], n_depth_cloud=s[2], used_total=s[3])

    def set_cloud(self, cloud):
        pts = A.as_pts(cloud)
        self.lib.check(self.lib.dll.lvi_depth_set_cloud(self._h, A._ptr(pts), len(pts)), "lvi_depth_set_cloud")

    def get_cloud(self):
        n = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_depth_get_cloud(self._h, None, 0, C.byref(n)), "lvi_depth_get_cloud")
        out = np.zeros(max(n.value, 1), A.PT_DTYPE)
        self.lib.check(self.lib.dll.lvi_depth_get_cloud(self._h, A._ptr(out), n.value, C.byref(n)), "lvi_depth_get_cloud")
        return out[:n.value].copy()

    def debug_voxel(self):
        n = C.c_int32(0)
        self.lib.check(self.lib.dll.lvi_depth_debug_voxel(self._h, None, None, 0, C.byref(n)), "lvi_depth_debug_voxel")
        cells = np.zeros(max(n.value, 1), np.int32); counts = np.zeros(max(n.value, 1), np.int32)
        self.lib.check(self.lib.dll.lvi_depth_debug_voxel(self._h, A._ptr(cells), A._ptr(counts), n.value, C.byref(n)), "lvi_depth_debug_voxel")
        return cells[:n.value].copy(), counts[:n.value].copy()

    def debug_range(self):
        sel = np.zeros(NUM_BINS * NUM_BINS, np.int32)
        self.lib.check(self.lib.dll.lvi_depth_debug_range(self._h, A._ptr(sel)), "lvi_depth_debug_range")
        return sel.reshape(NUM_BINS, NUM_BINS)

    def debug_sphere(self):
        n = C.c_int32(0)
        out = np.zeros(NUM_BINS * NUM_BINS, A.PT_DTYPE)
        self.lib.check(self.lib.dll.lvi_depth_debug_sphere(self._h, A._ptr(out), len(out), C.byref(n)), "lvi_depth_debug_sphere")
        return out[:n.value].copy()

    def debug_neighbors(self):
        n = C.c_int32(0)
        idx = np.zeros((self.max_features, 3), np.int32); sqd = np.zeros((self.max_features, 3), np.float32)
        self.lib.check(self.lib.dll.lvi_depth_debug_neighbors(self._h, A._ptr(idx), A._ptr(sqd), self.max_features, C.byref(n)),
                       "lvi_depth_debug_neighbors")
        return idx[:n.value].copy(), sqd[:n.value].copy()

    def set_full_search(self, on):
        self.lib.check(self.lib.dll.lvi_depth_set_full_search(self._h, 1 if on else 0), "lvi_depth_set_full_search")
