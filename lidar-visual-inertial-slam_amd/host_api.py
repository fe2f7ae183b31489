"""ctypes view of host/lvi_seq_capi.cpp: the C++ host mirror (host/lvi_host.hpp — the reference's node classes over the
C-ABI) flattened to C for the replay harness: the sequential lidar_odometry loop and the feature_tracker node callback.

One binding, parameterised by the shared-library path: ``host/liblvi_host_hip.so`` (built by build.py, linked against
the product library) in deployment and bench; the CPU-tier tests build the same source against the CPU library they check with.
"""
import ctypes as C
import os
import subprocess
from shutil import which
from typing import NamedTuple

import numpy as np

from . import _abi as A
from .fman import FmanFrameInfo, FmanParams, FmanTriInfo
from .loop import LoopInfo
from .marg import MargInfo, MargParams
from .pgo import PgoInfo
from .win import WinInfo, WinParams

HOST_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
HOST_HIP_LIB = os.path.join(HOST_DIR, "liblvi_host_hip.so")


class SeqParams(C.Structure):
    _fields_ = [("incremental_map", C.c_int32), ("use_imu_heading_initialization", C.c_int32), ("mapping_process_interval", C.c_double),
                ("keyframe_adding_dist", C.c_float), ("keyframe_adding_angle", C.c_float), ("keyframe_density", C.c_float),
                ("keyframe_search_radius", C.c_float)]


class SeqResult(C.Structure):
    _fields_ = [("processed", C.c_int32), ("status", C.c_int32), ("iters", C.c_int32), ("converged", C.c_int32), ("degenerate", C.c_int32),
                ("saved_keyframe", C.c_int32), ("n_keyframes", C.c_int32), ("n_keys", C.c_int32), ("pose", C.c_float * 6)]


FUNDAMENTAL_FN = C.CFUNCTYPE(None, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, C.c_double, C.POINTER(C.c_uint8), C.c_void_p)


_P, _vp, _cp, _i32, _i64, _f32, _f64 = C.POINTER, C.c_void_p, C.c_char_p, C.c_int32, C.c_int64, C.c_float, C.c_double
_ip, _fp, _dp = _P(_i32), _P(_f32), _P(_f64)
_scan = [_vp, _vp, _i32, _f64, _i32, _f32, _f32, _f32, _P(SeqResult)]

# name -> (restype, argtypes) of host/lvi_seq_capi.cpp: in every host library, whatever it is linked against
CORE_SIGNATURES = {
    "lvh_last_error": (_cp, []),
    "lvh_seq_params_default": (None, [_P(SeqParams)]),
    "lvh_seq_create": (_vp, [_P(A.LidarParams), _i32, _P(SeqParams)]),
    "lvh_seq_destroy": (None, [_vp]),
    "lvh_seq_handle": (_vp, [_vp]),
    "lvh_seq_scan": (_i32, _scan),
    "lvh_seq_scan_device": (_i32, _scan),
    "lvh_seq_seed_keyframe": (_i32, [_vp, _vp, _i32, _vp, _i32, _fp, _f64]),
    "lvh_seq_keys": (_i32, [_vp, _vp, _i32, _ip]),
    "lvh_seq_keyposes": (_i32, [_vp, _vp, _i32, _ip]),
    "lvh_trk_create": (_vp, [_P(A.TrackerParams), _i32, _i32, _i32, _i32, _i32, _P(A.MeiParams)]),
    "lvh_trk_destroy": (None, [_vp]),
    "lvh_trk_set_fundamental_hook": (None, [_vp, FUNDAMENTAL_FN, _vp]),
    "lvh_trk_image": (_i32, [_vp, _vp, _f64, _ip, _ip, _vp, _vp, _i32, _ip]),
    "lvh_trk_points": (_i32, [_vp, _vp, _i32, _ip]),
}
# exported for the other translation units of the library only (they reach the node objects through these)
INTERNAL_EXPORTS = ("lvh_seq_node", "lvh_trk_node")


class Component(NamedTuple):
    """one optional part of the host mirror: include/lvi_X.h is exported by liblvi_hip.so only, so host/lvi_X_capi.cpp is
    linked into the HIP host library alone, never into one built against the CPU oracle"""
    sources: tuple          # under host/
    needs: tuple            # components whose sources go with it
    flag: str               # the HostLibrary attribute it sets ...
    probe: str              # ... when the library exports this
    last_error: str
    signatures: dict        # name -> (restype, argtypes), every export of `sources`


def _component(name, signatures, needs=(), flag=None, probe=None, err=None):
    last_error = f"lvh_{err or name}_last_error"
    return Component((f"lvi_{name}_capi.cpp",), tuple(needs), flag or "has_" + name, probe or f"lvh_{name}_create", last_error,
                     {last_error: (_cp, []), **signatures})


COMPONENTS = {
    "depth": _component("depth", {
        "lvh_depth_create": (_vp, [_i32, _i32, _i32, _i32, _i32, _f64]),
        "lvh_depth_destroy": (None, [_vp]),
        "lvh_depth_handle": (_vp, [_vp]),
        "lvh_depth_install": (_i32, [_vp, _vp]),
        "lvh_depth_lidar": (_i32, [_vp, _vp, _i32, _fp, _f64, _ip]),
        "lvh_depth_set_image_pose": (_i32, [_vp, _fp]),
    }),
    # the device RANSAC behind a TrackerNode's rejectWithF
    "fmat": _component("fmat", {
        "lvh_trk_use_device_fundamental": (_i32, [_vp, _i32]),
    }, probe="lvh_trk_use_device_fundamental"),
    "gmap": _component("gmap", {
        "lvh_gmap_create": (_vp, [_vp, _f32, _f32, _f32]),
        "lvh_gmap_destroy": (None, [_vp]),
        "lvh_gmap_reserve": (_i32, [_vp, _i32]),
        "lvh_gmap_keys": (_i32, [_vp, _vp, _i32, _ip]),
        "lvh_gmap_publish": (_i32, [_vp, _ip]),
        "lvh_gmap_cloud": (_i32, [_vp, _vp, _i32, _ip]),
        "lvh_gmap_save": (_i32, [_vp, _cp, _f32]),
    }),
    "loop": _component("loop", {
        "lvh_loop_create": (_vp, [_vp, _f32, _f32, _i32, _f32, _f32, _i32]),
        "lvh_loop_destroy": (None, [_vp]),
        "lvh_loop_reserve": (_i32, [_vp, _i32, _i32]),
        "lvh_loop_info_msg": (_i32, [_vp, _dp, _i32]),
        "lvh_loop_detect": (_i32, [_vp, _i32, _f64, _ip]),
        "lvh_loop_start": (_i32, [_vp, _f64]),
        "lvh_loop_finish": (_i32, [_vp, _P(LoopInfo)]),
        "lvh_loop_queue_size": (_i32, [_vp]),
        "lvh_loop_pop": (_i32, [_vp, _ip, _dp, _fp]),
        "lvh_loop_closed": (_i32, [_vp, _vp, _i32, _ip]),
        "lvh_loop_cloud": (_i32, [_vp, _i32, _vp, _i32, _ip]),
    }),
    "kf": _component("kf", {
        "lvh_kf_create": (_vp, [_i32] * 6 + [_ip] * 4),
        "lvh_kf_destroy": (None, [_vp]),
        "lvh_kf_handle": (_vp, [_vp]),
        "lvh_kf_add": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _P(A.MeiParams), _ip]),
        "lvh_kf_remove": (_i32, [_vp, _i32]),
        "lvh_kf_connect": (_i32, [_vp, _i32, _i32, _ip]),
        "lvh_kf_connection": (_i32, [_vp] * 8 + [_i32]),
    }),
    "bow": _component("bow", {
        "lvh_bow_create": (_vp, [_i32] * 6 + [_ip] * 4 + [_i32]),
        "lvh_bow_destroy": (None, [_vp]),
        "lvh_bow_kf_handle": (_vp, [_vp]),
        "lvh_bow_db_handle": (_vp, [_vp]),
        "lvh_bow_load_vocabulary": (_i32, [_vp, _cp]),
        "lvh_bow_add_keyframe": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _ip, _vp]),
        "lvh_bow_connection": (_i32, [_vp, _vp, _vp, _vp]),
    }),
    # it hooks into the loop detector
    "pnp": _component("pnp", {
        "lvh_pnp_create": (_vp, [_i32, _i32, _i32]),
        "lvh_pnp_destroy": (None, [_vp]),
        "lvh_pnp_handle": (_vp, [_vp]),
        "lvh_pnp_status": (_i32, [_vp, _vp, _vp, _i32, _vp]),
        "lvh_bow_use_pnp": (_i32, [_vp, _vp]),
        "lvh_bow_pnp_connection": (_i32, [_vp, _vp, _vp, _vp]),
    }, needs=("bow",)),
    # it reads the loop closer's constraints
    "pgo": _component("pgo", {
        "lvh_pgo_create": (_vp, [_i32, _i32, _i32, _i32, _i32, _f64]),
        "lvh_pgo_destroy": (None, [_vp]),
        "lvh_pgo_handle": (_vp, [_vp]),
        "lvh_seq_use_pose_graph": (_i32, [_vp, _vp]),
        "lvh_pgo_push_loop": (_i32, [_vp, _i32, _i32, _dp, _f32]),
        "lvh_pgo_last": (_i32, [_vp, _P(PgoInfo), _fp, _ip]),
        "lvh_seq_poses_corrected": (_i32, [_vp]),
        "lvh_seq_use_gps": (_i32, [_vp, _i32, _f32, _f32]),
        "lvh_seq_gps_push": (_i32, [_vp, _f64, _dp, _dp]),
        "lvh_seq_gps_last": (_i32, [_vp, _dp, _ip]),
    }, needs=("loop",)),
    # the camera rig; its cameras may take the device RANSAC
    "tbatch": _component("tbatch", {
        "lvh_rig_create": (_vp, [_P(A.TrackerParams), _i32, _i32, _i32, _i32, _i32, _P(A.MeiParams), _i32]),
        "lvh_rig_destroy": (None, [_vp]),
        "lvh_rig_use_device_fundamental": (_i32, [_vp, _i32]),
        "lvh_rig_use_batched_fundamental": (_i32, [_vp, _i32]),
        "lvh_rig_fundamental_stats": (_i32, [_vp, _P(_i64)]),
        "lvh_rig_read_images": (_i32, [_vp, _P(_vp), _dp, _ip]),
        "lvh_rig_update_ids": (_i32, [_vp]),
        "lvh_rig_reset_ids": (None, []),
        "lvh_rig_camera": (_i32, [_vp, _i32, _vp, _vp, _i32, _ip]),
    }, needs=("fmat",), flag="has_rig", probe="lvh_rig_create", err="rig"),
    "marg": _component("marg", {
        "lvh_marg_create": (_vp, [_i32, _i32, _i32, _P(MargParams)]),
        "lvh_marg_destroy": (None, [_vp]),
        "lvh_marg_handle": (_vp, [_vp]),
        "lvh_marg_set_window": (_i32, [_vp, _dp, _dp, _dp, _f64]),
        "lvh_marg_set_features": (_i32, [_vp, _i32, _ip, _ip, _dp, _dp]),
        "lvh_marg_set_imu": (_i32, [_vp, _f64, _dp, _dp]),
        "lvh_marg_run": (_i32, [_vp, _i32, _ip, _P(MargInfo)]),
    }),
    # it optimises the marginaliser's window arrays
    "win": _component("win", {
        "lvh_win_create": (_vp, [_vp, _i32, _i32, _i32, _i32, _f64, _P(WinParams)]),
        "lvh_win_destroy": (None, [_vp]),
        "lvh_win_handle": (_vp, [_vp]),
        "lvh_win_set_imu": (_i32, [_vp, _i32, _vp]),
        "lvh_win_set_lidar_flags": (_i32, [_vp, _i32, _ip]),
        "lvh_win_optimize": (_i32, [_vp, _i32, _P(WinInfo)]),
        "lvh_win_get_window": (_i32, [_vp, _dp, _dp, _dp, _dp, _i32, _ip, _dp]),
    }, needs=("marg",)),
    # fillWindow writes into both
    "fman": _component("fman", {
        "lvh_fman_create": (_vp, [_i32, _i32, _P(FmanParams)]),
        "lvh_fman_destroy": (None, [_vp]),
        "lvh_fman_handle": (_vp, [_vp]),
        "lvh_fman_clear_state": (_i32, [_vp]),
        "lvh_fman_add_frame": (_i32, [_vp, _i32, _i32, _ip, _dp, _f64, _P(FmanFrameInfo)]),
        "lvh_fman_triangulate": (_i32, [_vp, _dp, _dp, _dp, _dp, _P(FmanTriInfo)]),
        "lvh_fman_fill_window": (_i32, [_vp, _vp, _vp]),
        "lvh_fman_take_depths": (_i32, [_vp, _vp]),
        "lvh_fman_remove_failures": (_i32, [_vp]),
        "lvh_fman_slide_old": (_i32, [_vp, _i32, _dp, _dp, _dp, _dp, _dp, _dp]),
        "lvh_fman_slide_new": (_i32, [_vp, _i32]),
    }, needs=("marg", "win")),
}


def component_sources(names=None):
    """the source files of the named components and of everything they need, each once, in table order (None: all)"""
    want, todo = set(), list(COMPONENTS if names is None else names)
    while todo:
        name = todo.pop()
        if name not in want:
            want.add(name)
            todo += COMPONENTS[name].needs
    return tuple(f for name, c in COMPONENTS.items() if name in want for f in c.sources)


def host_dependencies(sources=()):
    """what a host library of these sources is rebuilt for: its .cpp files, every host/*.hpp and every include/*.h (no
    host file includes anything else of the project's)"""
    inc = os.path.normpath(os.path.join(HOST_DIR, "..", "..", "include"))
    return ([os.path.join(HOST_DIR, f) for f in ("lvi_seq_capi.cpp", *sources)]
            + sorted(os.path.join(HOST_DIR, f) for f in os.listdir(HOST_DIR) if f.endswith(".hpp"))
            + sorted(os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h")))


def build_host_library(out_path, link_dir, link_name, extra=(), sources=()):
    """g++ -shared of host/lvi_seq_capi.cpp (+ the named host/ sources) against lib<link_name>.so in link_dir (rpath set)"""
    if os.path.exists(out_path) and all(os.path.getmtime(d) <= os.path.getmtime(out_path) for d in host_dependencies(sources)):
        return out_path
    srcs = [os.path.join(HOST_DIR, f) for f in ("lvi_seq_capi.cpp", *sources)]
    cxx = which("g++") or "g++"
    cmd = [cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", out_path, *srcs, "-L" + link_dir, "-l" + link_name,
           "-Wl,-rpath," + link_dir, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("host library build failed:\n" + r.stdout + r.stderr)
    return out_path


class HostLibrary:
    bind = A.Library.bind

    def __init__(self, path):
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found — build it first (python -c 'import __graft_entry__ as g; g.build()')")
        self.dll = C.CDLL(path, mode=getattr(os, "RTLD_LOCAL", 0) | getattr(os, "RTLD_NOW", 2))
        self._bound = set()
        self.bind(CORE_SIGNATURES)
        for c in COMPONENTS.values():                    # has_depth ... has_fman: the HIP host library only
            present = hasattr(self.dll, c.probe)
            if present:
                self.bind(c.signatures)
            setattr(self, c.flag, present)

    def check(self, code, where):
        if code < 0:
            raise A.LviError(code, where, self.dll.lvh_last_error().decode(errors="replace"))
        return code


class _HostOwned(A.Owned):
    _lib = "hl"


class _BorrowedHandle:
    """a LidarHotpath-like view of the lvi_lidar owned by the C++ side (never destroyed from here)"""

    def __init__(self, lidar_cls, lib, ptr, params):
        self._obj = lidar_cls.__new__(lidar_cls)
        self._obj.lib, self._obj.params, self._obj._h = lib, params, C.c_void_p(ptr)
        self._obj._cap_scan = int(params.N_SCAN) * int(params.Horizon_SCAN)
        self._obj.close = lambda: None

    def __getattr__(self, k):
        return getattr(self._obj, k)


class SequentialMapper(_HostOwned):
    """MapOptimizationNode of host/lvi_host.hpp (updateInitialGuess, extractNearby, extractCloud, scan matching, saveFrame,
    key-pose push; mapOptimization.cpp:298-333, 806-999, 1315-1412, 1529-1603) fed scan by scan"""
    _ptr, _destroy, _last_error = "_s", "lvh_seq_destroy", "lvh_last_error"

    def __init__(self, hostlib, abi_lib, lidar_params, device=0, **seq):
        from .lidar import LidarHotpath
        self.hl = hostlib
        sp = SeqParams()
        hostlib.dll.lvh_seq_params_default(C.byref(sp))
        for k, v in seq.items():
            if not hasattr(sp, k):
                raise AttributeError(f"lvh_seq_params has no field {k}")
            setattr(sp, k, v)
        self.seq_params = sp
        self._s = hostlib.dll.lvh_seq_create(C.byref(lidar_params), int(device), C.byref(sp))
        if not self._s:
            raise A.LviError(-3, "lvh_seq_create", hostlib.dll.lvh_last_error().decode(errors="replace"))
        self.handle = _BorrowedHandle(LidarHotpath, abi_lib, hostlib.dll.lvh_seq_handle(self._s), lidar_params)

    @staticmethod
    def _res(r):
        return dict(processed=bool(r.processed), status=r.status, iters=r.iters, converged=bool(r.converged), degenerate=bool(r.degenerate),
                    saved_keyframe=bool(r.saved_keyframe), n_keyframes=r.n_keyframes, n_keys=r.n_keys, pose=np.array(r.pose[:], np.float32))

    def scan(self, livox_pts, stamp, imu=None):
        pts = np.ascontiguousarray(livox_pts, dtype=A.LIVOX_DTYPE)
        r = SeqResult()
        ia, ro, pi, ya = (1, imu[0], imu[1], imu[2]) if imu is not None else (0, 0.0, 0.0, 0.0)
        self.hl.check(self.hl.dll.lvh_seq_scan(self._s, A._ptr(pts), len(pts), float(stamp), ia, ro, pi, ya, C.byref(r)), "lvh_seq_scan")
        return self._res(r)

    def scan_device(self, d_ptr, n_raw, stamp, imu=None):
        r = SeqResult()
        ia, ro, pi, ya = (1, imu[0], imu[1], imu[2]) if imu is not None else (0, 0.0, 0.0, 0.0)
        self.hl.check(self.hl.dll.lvh_seq_scan_device(self._s, C.c_void_p(int(d_ptr)), int(n_raw), float(stamp), ia, ro, pi, ya, C.byref(r)), "lvh_seq_scan_device")
        return self._res(r)

    def seed_keyframe(self, corner, surf, pose, time):
        """a keyframe of an earlier session: DS clouds (sensor frame) into the device store, pose into the key poses"""
        c, s = A.as_pts(corner), A.as_pts(surf)
        pose_c = (C.c_float * 6)(*[float(v) for v in pose])
        return self.hl.check(self.hl.dll.lvh_seq_seed_keyframe(self._s, A._ptr(c), len(c), A._ptr(s), len(s), pose_c, float(time)), "lvh_seq_seed_keyframe")

    def usePoseGraph(self, backend):
        """MapOptimizationNode::usePoseGraph: the node applies loop closures through this PoseGraphBackend (prior / odometry
        edge per key, the pushed loop constraints, a solve when one was added, correctPoses); None removes the hook.  Install
        it before the first key.  keyposes() then returns the corrected key poses."""
        if not self.hl.has_pgo:
            raise RuntimeError("this host library has no pose-graph back end (only the one linked against liblvi_hip.so has)")
        code = self.hl.dll.lvh_seq_use_pose_graph(self._s, backend._p if backend is not None else None)
        if code < 0:
            raise A.LviError(code, "lvh_seq_use_pose_graph", self.hl.dll.lvh_pgo_last_error().decode(errors="replace"))
        self._pg = backend                                               # keeps it alive while installed

    def useGps(self, use_gps_elevation=False, gps_cov_threshold=2.0, pose_cov_threshold=25.0):
        """MapOptimizationNode::useGps (addGPSFactor, mapOptimization.cpp:1430-1507, with the settings of utility.h:178-183; the
        keyword arguments are config.load_gps_yaml's): on top of usePoseGraph, a key may take one GPS factor from the messages
        pushed with gpsHandler, and the newest key's marginal covariance is stored after every key"""
        if not self.hl.has_pgo:
            raise RuntimeError("this host library has no pose-graph back end (only the one linked against liblvi_hip.so has)")
        code = self.hl.dll.lvh_seq_use_gps(self._s, int(bool(use_gps_elevation)), float(gps_cov_threshold), float(pose_cov_threshold))
        if code < 0:
            raise A.LviError(code, "lvh_seq_use_gps", self.hl.dll.lvh_pgo_last_error().decode(errors="replace"))

    def gpsHandler(self, stamp, xyz, cov_xyz):
        """gpsHandler (:334-337): one odometry message's stamp, position and covariance[0], [7], [14] -> the queue's length"""
        z = (C.c_double * 3)(*[float(v) for v in xyz])
        c = (C.c_double * 3)(*[float(v) for v in cov_xyz])
        return int(self.hl.dll.lvh_seq_gps_push(self._s, float(stamp), z, c))

    def gps_last(self):
        """dict(pose_covariance [6, 6] (:1591), factors_added, queued, in_use)"""
        cov, cnt = np.zeros(36, np.float64), (C.c_int32 * 3)()
        self.hl.dll.lvh_seq_gps_last(self._s, cov.ctypes.data_as(C.POINTER(C.c_double)), cnt)
        return dict(pose_covariance=cov.reshape(6, 6), factors_added=cnt[0], queued=cnt[1], in_use=bool(cnt[2]))

    def poses_corrected(self):
        """how often correctPoses rewrote the key poses"""
        if not self.hl.has_pgo:
            return 0
        return int(self.hl.dll.lvh_seq_poses_corrected(self._s))

    def keys(self):
        n = C.c_int32(0)
        self.hl.check(self.hl.dll.lvh_seq_keys(self._s, None, 0, C.byref(n)), "lvh_seq_keys")
        out = np.zeros(max(n.value, 1), np.int32)
        self.hl.check(self.hl.dll.lvh_seq_keys(self._s, A._ptr(out), len(out), C.byref(n)), "lvh_seq_keys")
        return out[:n.value].copy()

    def keyposes(self):
        n = C.c_int32(0)
        self.hl.check(self.hl.dll.lvh_seq_keyposes(self._s, None, 0, C.byref(n)), "lvh_seq_keyposes")
        out = np.zeros((max(n.value, 1), 8), np.float64)
        self.hl.check(self.hl.dll.lvh_seq_keyposes(self._s, A._ptr(out), len(out), C.byref(n)), "lvh_seq_keyposes")
        return out[:n.value].copy()


class TrackerNode(_HostOwned):
    """FeatureTrackerNode of host/lvi_host.hpp: img_callback of feature_tracker_node.cpp:37-231 without ROS"""
    _ptr, _destroy, _last_error = "_t", "lvh_trk_destroy", "lvh_last_error"
    OUTCOMES = ("first_image", "restart", "not_published", "first_publish_suppressed", "published")

    def __init__(self, hostlib, tracker_params, row, col, freq, equalize=False, cam=None, device=0):
        self.hl = hostlib
        c = A.MeiParams(*[float(cam[k]) for k in ("xi", "k1", "k2", "p1", "p2", "gamma1", "gamma2", "u0", "v0")]) if cam is not None else None
        self._t = hostlib.dll.lvh_trk_create(C.byref(tracker_params), int(device), int(row), int(col), int(freq), 1 if equalize else 0,
                                             C.byref(c) if c is not None else None)
        if not self._t:
            raise A.LviError(-3, "lvh_trk_create", hostlib.dll.lvh_last_error().decode(errors="replace"))
        self.cap = int(tracker_params.max_features)
        self._hook = None

    def set_fundamental_hook(self, fn):
        """fn(un_cur [n,2], un_forw [n,2], f_threshold) -> status [n] (uint8): the node's cv::findFundamentalMat"""
        if fn is None:
            self._hook = None
            self.hl.dll.lvh_trk_set_fundamental_hook(self._t, C.cast(None, FUNDAMENTAL_FN), None)
            return

        def tramp(a, b, n, thr, status, _user):
            ua = np.ctypeslib.as_array(a, shape=(n, 2)).copy() if n else np.zeros((0, 2), np.float32)
            ub = np.ctypeslib.as_array(b, shape=(n, 2)).copy() if n else np.zeros((0, 2), np.float32)
            st = np.asarray(fn(ua, ub, thr), np.uint8)
            for i in range(n):
                status[i] = int(st[i])
        self._hook = FUNDAMENTAL_FN(tramp)
        self.hl.dll.lvh_trk_set_fundamental_hook(self._t, self._hook, None)

    def use_device_fundamental(self, device=0):
        """rejectWithF's findFundamentalMat := the device RANSAC (lvi_host::DeviceFundamental, include/lvi_fmat.h).  HIP
        host library only; set_fundamental_hook replaces it again."""
        if not self.hl.has_fmat:
            raise RuntimeError("this host library has no device RANSAC (only the one linked against liblvi_hip.so has)")
        code = self.hl.dll.lvh_trk_use_device_fundamental(self._t, int(device))
        if code < 0:
            raise A.LviError(code, "lvh_trk_use_device_fundamental", self.hl.dll.lvh_fmat_last_error().decode(errors="replace"))
        self._hook = None

    def image(self, img, stamp):
        img = np.ascontiguousarray(img, np.uint8)
        oc, n = C.c_int32(0), C.c_int32(0)
        pts = np.zeros((self.cap, 3), np.float32)
        ch = np.zeros((6, self.cap), np.float32)
        info = (C.c_int32 * 4)()
        self.hl.check(self.hl.dll.lvh_trk_image(self._t, A._ptr(img), float(stamp), C.byref(oc), C.byref(n), A._ptr(pts), A._ptr(ch), self.cap, info),
                      "lvh_trk_image")
        m = n.value
        return dict(outcome=self.OUTCOMES[oc.value], points=pts[:m].copy(), channels=ch[:, :m].copy(), pub_this_frame=bool(info[0]),
                    rejectWithF_skipped=info[1], n_cur_pts=info[2], pub_count=info[3])

    def points(self):
        n = C.c_int32(0)
        rows = np.zeros((self.cap, 4), np.float32)
        self.hl.check(self.hl.dll.lvh_trk_points(self._t, A._ptr(rows), self.cap, C.byref(n)), "lvh_trk_points")
        return rows[:n.value].copy()


class NodeDepthRegister(_HostOwned):
    """lvi_host::DepthRegister (host/lvi_depth_host.hpp) installed as the get_depth of a TrackerNode: the node's
    lidar_callback (feature_tracker_node.cpp:273-377) and the depth channel of its messages.  pose6 = (x, y, z, roll,
    pitch, yaw) of the body in the world frame, or None for a failed TF lookup.  HIP host library only."""
    _ptr, _destroy, _last_error = "_d", "lvh_depth_destroy", "lvh_depth_last_error"

    def __init__(self, hostlib, node, abi_lib, device=0, max_clouds=64, max_cloud_points=131072, max_features=150, lidar_skip=3, window_s=5.0):
        from .depth import DepthRegister, bind as depth_bind
        if not hostlib.has_depth:
            raise RuntimeError("this host library has no depth register (only the one linked against liblvi_hip.so has)")
        self.hl = hostlib
        self._d = hostlib.dll.lvh_depth_create(int(device), int(max_clouds), int(max_cloud_points), int(max_features), int(lidar_skip), float(window_s))
        if not self._d:
            raise A.LviError(-3, "lvh_depth_create", hostlib.dll.lvh_depth_last_error().decode(errors="replace"))
        self._check(hostlib.dll.lvh_depth_install(self._d, node._t), "lvh_depth_install")
        self.node = node
        # a DepthRegister view of the handle the C++ side owns (debug views; never destroyed from here)
        self.register = DepthRegister.__new__(DepthRegister)
        self.register.lib = depth_bind(abi_lib)
        self.register.max_features, self.register.max_cloud_points, self.register.max_clouds = int(max_features), int(max_cloud_points), int(max_clouds)
        self.register._h = C.c_void_p(hostlib.dll.lvh_depth_handle(self._d))
        self.register.close = lambda: None

    @staticmethod
    def _pose(pose6):
        return None if pose6 is None else (C.c_float * 6)(*[float(v) for v in np.asarray(pose6, np.float32).reshape(6)])

    def lidar_callback(self, cloud, pose6, stamp):
        pts = A.as_pts(cloud)
        used = C.c_int32(0)
        self._check(self.hl.dll.lvh_depth_lidar(self._d, A._ptr(pts), len(pts), self._pose(pose6), float(stamp), C.byref(used)), "lvh_depth_lidar")
        return bool(used.value)

    def set_image_pose(self, pose6):
        """the transform the next image's get_depth reads (the reference's TF lookup at Time(0))"""
        self._check(self.hl.dll.lvh_depth_set_image_pose(self._d, self._pose(pose6)), "lvh_depth_set_image_pose")


class GlobalMapper(_HostOwned):
    """lvi_host::GlobalMapper (host/lvi_gmap_host.hpp) over a SequentialMapper's node: publishGlobalMap
    (mapOptimization.cpp:460-510) and the save_map service (:179-236).  HIP host library only."""
    _ptr, _destroy, _last_error = "_g", "lvh_gmap_destroy", "lvh_gmap_last_error"

    def __init__(self, hostlib, mapper, search_radius=1000.0, pose_density=1.0, leaf_size=0.05):
        if not hostlib.has_gmap:
            raise RuntimeError("this host library has no global mapper (only the one linked against liblvi_hip.so has)")
        self.hl = hostlib
        self._g = hostlib.dll.lvh_gmap_create(mapper._s, float(search_radius), float(pose_density), float(leaf_size))
        if not self._g:
            raise A.LviError(-1, "lvh_gmap_create", hostlib.dll.lvh_gmap_last_error().decode(errors="replace"))

    def reserve(self, max_points):
        self._check(self.hl.dll.lvh_gmap_reserve(self._g, int(max_points)), "lvh_gmap_reserve")

    def keys(self):
        """publishGlobalMap steps 2-6: the key clouds of globalMapKeyFrames in fuse order"""
        n = C.c_int32(0)
        self._check(self.hl.dll.lvh_gmap_keys(self._g, None, 0, C.byref(n)), "lvh_gmap_keys")
        out = np.zeros(max(n.value, 1), np.int32)
        self._check(self.hl.dll.lvh_gmap_keys(self._g, A._ptr(out), len(out), C.byref(n)), "lvh_gmap_keys")
        return out[:n.value].copy()

    def publishGlobalMap(self):
        """the published cloud and dict(n_fused, n_out, overflow, filtered); None when there are no key poses"""
        info = (C.c_int32 * 4)()
        if self._check(self.hl.dll.lvh_gmap_publish(self._g, info), "lvh_gmap_publish") == 0:
            return None
        n = C.c_int32(0)
        self._check(self.hl.dll.lvh_gmap_cloud(self._g, None, 0, C.byref(n)), "lvh_gmap_cloud")
        out = np.zeros(max(n.value, 1), A.PT_DTYPE)
        self._check(self.hl.dll.lvh_gmap_cloud(self._g, A._ptr(out), len(out), C.byref(n)), "lvh_gmap_cloud")
        return out[:n.value].copy(), dict(n_fused=info[0], n_out=info[1], overflow=bool(info[2]), filtered=bool(info[3]))

    def saveMap(self, directory, resolution):
        """the save_map service: five binary PCD files in `directory`; returns its `success`"""
        return bool(self._check(self.hl.dll.lvh_gmap_save(self._g, os.fsencode(str(directory)), float(resolution)), "lvh_gmap_save"))


class LoopCloser(_HostOwned):
    """lvi_host::LoopCloser (host/lvi_loop_host.hpp) over a SequentialMapper's node: the loop-closure thread of
    mapOptimization.cpp (:523-741) up to the constraint queue.  HIP host library only."""
    _ptr, _destroy, _last_error = "_g", "lvh_loop_destroy", "lvh_loop_last_error"

    def __init__(self, hostlib, mapper, search_radius=15.0, search_time_diff=30.0, search_num=25, fitness_score=0.3, surf_leaf=0.4,
                 incremental_cloud=1, **_ignored):
        if not hostlib.has_loop:
            raise RuntimeError("this host library has no loop closer (only the one linked against liblvi_hip.so has)")
        self.hl = hostlib
        self._g = hostlib.dll.lvh_loop_create(mapper._s, float(search_radius), float(search_time_diff), int(search_num), float(fitness_score),
                                              float(surf_leaf), int(incremental_cloud))
        if not self._g:
            raise A.LviError(-1, "lvh_loop_create", hostlib.dll.lvh_loop_last_error().decode(errors="replace"))

    def reserve(self, max_source_points, max_target_points):
        self._check(self.hl.dll.lvh_loop_reserve(self._g, int(max_source_points), int(max_target_points)), "lvh_loop_reserve")

    def loopInfoHandler(self, data):
        """a loop-info message (kept only when it holds two values); returns the queue's length"""
        d = np.ascontiguousarray(data, np.float64).reshape(-1)
        return self._check(self.hl.dll.lvh_loop_info_msg(self._g, d.ctypes.data_as(C.POINTER(C.c_double)), len(d)), "lvh_loop_info_msg")

    def _detect(self, which, t):
        keys = (C.c_int32 * 2)(-1, -1)
        ok = self._check(self.hl.dll.lvh_loop_detect(self._g, which, float(t), keys), "lvh_loop_detect")
        return (keys[0], keys[1]) if ok else None

    def detectLoopClosureDistance(self, time_laser_info_cur):
        """(cur, pre) or None, on fresh copies of the node's key poses"""
        return self._detect(0, time_laser_info_cur)

    def detectLoopClosureExternal(self):
        return self._detect(1, 0.0)

    def startLoop(self, time_laser_info_cur):
        """the key search and the enqueue of the device job; False when no loop was found"""
        return bool(self._check(self.hl.dll.lvh_loop_start(self._g, float(time_laser_info_cur)), "lvh_loop_start"))

    def finishLoop(self):
        """(pushed, info): waits for the job, applies the gates and pushes the constraint"""
        from .loop import LoopInfo
        r = LoopInfo()
        ok = bool(self._check(self.hl.dll.lvh_loop_finish(self._g, C.byref(r)), "lvh_loop_finish"))
        info = {k: getattr(r, k) for k, _ in LoopInfo._fields_ if k != "transformation"}
        info["transformation"] = np.array(r.transformation, np.float32).reshape(4, 4)
        return ok, info

    def performLoopClosure(self, time_laser_info_cur):
        if not self.startLoop(time_laser_info_cur):
            return False, None
        return self.finishLoop()

    def queue_size(self):
        return int(self.hl.dll.lvh_loop_queue_size(self._g))

    def pop(self):
        """the oldest constraint: dict(key_cur, key_pre, between [4, 4] float64, noise) or None"""
        keys = (C.c_int32 * 2)()
        b = np.zeros(16, np.float64)
        noise = C.c_float(0)
        if not self._check(self.hl.dll.lvh_loop_pop(self._g, keys, b.ctypes.data_as(C.POINTER(C.c_double)), C.byref(noise)), "lvh_loop_pop"):
            return None
        return dict(key_cur=keys[0], key_pre=keys[1], between=b.reshape(4, 4), noise=float(noise.value))

    def closed(self):
        """loopIndexContainer as {cur: pre}"""
        n = C.c_int32(0)
        self._check(self.hl.dll.lvh_loop_closed(self._g, None, 0, C.byref(n)), "lvh_loop_closed")
        out = np.zeros((max(n.value, 1), 2), np.int32)
        self._check(self.hl.dll.lvh_loop_closed(self._g, A._ptr(out), len(out), C.byref(n)), "lvh_loop_closed")
        return {int(a): int(b) for a, b in out[:n.value]}

    def cloud(self, what):
        """the target submap (loop.TARGET, pubHistoryKeyFrames) or the aligned source (loop.ALIGNED, pubIcpKeyFrames) of the last job"""
        n = C.c_int32(0)
        self._check(self.hl.dll.lvh_loop_cloud(self._g, int(what), None, 0, C.byref(n)), "lvh_loop_cloud")
        out = np.zeros(max(n.value, 1), A.PT_DTYPE)
        self._check(self.hl.dll.lvh_loop_cloud(self._g, int(what), A._ptr(out), len(out), C.byref(n)), "lvh_loop_cloud")
        return out[:n.value].copy()


class KeyFrameMatcher(_HostOwned):
    """lvi_host::KeyFrameDescriber (host/lvi_kf_host.hpp) with the host halves of its keyframes: the online KeyFrame
    constructor (keyframe.cpp:14-73) and findConnection up to PnPRANSAC (:179-200).  HIP host library only."""
    _ptr, _destroy, _last_error = "_m", "lvh_kf_destroy", "lvh_kf_last_error"

    def __init__(self, hostlib, pattern, device=0, max_width=1024, max_height=576, max_keypoints=8192, max_window=1024, max_keyframes=16):
        if not hostlib.has_kf:
            raise RuntimeError("this host library has no keyframe describer (only the one linked against liblvi_hip.so has)")
        self.hl = hostlib
        self.max_window = int(max_window)
        pat = [np.ascontiguousarray(p, np.int32).reshape(-1) for p in pattern]
        if len(pat) != 4 or any(len(p) != 256 for p in pat):
            raise ValueError("the BRIEF pattern is four arrays of 256 ints")
        self._m = hostlib.dll.lvh_kf_create(int(device), int(max_width), int(max_height), int(max_keypoints), self.max_window, int(max_keyframes),
                                            *[p.ctypes.data_as(C.POINTER(C.c_int32)) for p in pat])
        if not self._m:
            raise A.LviError(-1, "lvh_kf_create", hostlib.dll.lvh_kf_last_error().decode(errors="replace"))

    def add(self, slot, img, point_3d, point_2d_uv, point_2d_norm, point_id, cam=None):
        """the online KeyFrame constructor into `slot` -> dict(n_keypoints_found, n_keypoints_stored)"""
        from .kf import mei_params
        img = np.ascontiguousarray(img, np.uint8)
        p3 = np.ascontiguousarray(point_3d, np.float32).reshape(-1, 3)
        uv = np.ascontiguousarray(point_2d_uv, np.float32).reshape(-1, 2)
        nm = np.ascontiguousarray(point_2d_norm, np.float32).reshape(-1, 2)
        ids = np.ascontiguousarray(point_id, np.float64).reshape(-1)
        if not len(p3) == len(uv) == len(nm) == len(ids):
            raise ValueError("the window vectors differ in length")
        c = mei_params(cam)
        info = (C.c_int32 * 2)()
        self._check(self.hl.dll.lvh_kf_add(self._m, int(slot), A._ptr(img), img.shape[1], img.shape[0], img.shape[1], len(uv), A._ptr(p3), A._ptr(uv),
                                           A._ptr(nm), A._ptr(ids), C.byref(c) if c is not None else None, info), "lvh_kf_add")
        return dict(n_keypoints_found=info[0], n_keypoints_stored=info[1])

    def remove(self, slot):
        self._check(self.hl.dll.lvh_kf_remove(self._m, int(slot)), "lvh_kf_remove")

    def findConnectionFront(self, cur_slot, old_slot):
        """(passes the > MIN_LOOP_NUM gate, dict of the six compacted vectors PnPRANSAC would receive + searchByBRIEFDes's status)"""
        n = C.c_int32(0)
        ok = bool(self._check(self.hl.dll.lvh_kf_connect(self._m, int(cur_slot), int(old_slot), C.byref(n)), "lvh_kf_connect"))
        k = max(n.value, 1)
        v2 = [np.zeros((k, 2), np.float32) for _ in range(4)]
        p3 = np.zeros((k, 3), np.float32); ids = np.zeros(k, np.float64); st = np.zeros(self.max_window, np.uint8)
        self._check(self.hl.dll.lvh_kf_connection(self._m, *[A._ptr(a) for a in v2], A._ptr(p3), A._ptr(ids), A._ptr(st), len(st)), "lvh_kf_connection")
        m = n.value
        return ok, dict(matched_2d_cur=v2[0][:m].copy(), matched_2d_old=v2[1][:m].copy(), matched_2d_cur_norm=v2[2][:m].copy(),
                        matched_2d_old_norm=v2[3][:m].copy(), matched_3d=p3[:m].copy(), matched_id=ids[:m].copy(), status=st)


class LoopDetector(_HostOwned):
    """lvi_host::LoopDetector (host/lvi_bow_host.hpp) with a keyframe store of its own: LoopDetector::loadVocabulary and
    addKeyFrame of pose_graph/src/loop_detector.cpp (:6-40, 56-154) over the device database of include/lvi_bow.h.  HIP
    host library only.  `store` is a kf.KeyframeDescriber view of the store the C++ side owns: fill a slot through it
    (describe or put), then hand the keyframe's host half to addKeyFrame."""
    _ptr, _destroy, _last_error = "_d", "lvh_bow_destroy", "lvh_bow_last_error"

    def __init__(self, hostlib, abi_lib, pattern, max_entries=4096, device=0, max_width=1024, max_height=576, max_keypoints=8192, max_window=1024,
                 max_keyframes=16):
        from .kf import KeyframeDescriber, bind as kf_bind
        if not hostlib.has_bow:
            raise RuntimeError("this host library has no loop detector (only the one linked against liblvi_hip.so has)")
        self.hl = hostlib
        pat = [np.ascontiguousarray(p, np.int32).reshape(-1) for p in pattern]
        if len(pat) != 4 or any(len(p) != 256 for p in pat):
            raise ValueError("the BRIEF pattern is four arrays of 256 ints")
        self._d = hostlib.dll.lvh_bow_create(int(device), int(max_width), int(max_height), int(max_keypoints), int(max_window), int(max_keyframes),
                                             *[p.ctypes.data_as(C.POINTER(C.c_int32)) for p in pat], int(max_entries))
        if not self._d:
            raise A.LviError(-1, "lvh_bow_create", hostlib.dll.lvh_bow_last_error().decode(errors="replace"))
        # a KeyframeDescriber view of the store the C++ side owns (never destroyed from here)
        self.store = KeyframeDescriber.__new__(KeyframeDescriber)
        self.store.lib = kf_bind(abi_lib)
        self.store.max_width, self.store.max_height = int(max_width), int(max_height)
        self.store.max_keypoints, self.store.max_window, self.store.max_keyframes = int(max_keypoints), int(max_window), int(max_keyframes)
        self.store._h = C.c_void_p(hostlib.dll.lvh_bow_kf_handle(self._d))
        self.store.close = lambda: None

    def loadVocabulary(self, path):
        """the vocabulary file in the VINSLoop layout (pose_graph_node.cpp:300-304); it is not shipped with the project"""
        self._check(self.hl.dll.lvh_bow_load_vocabulary(self._d, os.fsencode(str(path))), "lvh_bow_load_vocabulary")

    def addKeyFrame(self, slot, index, flag_detect_loop=True, point_3d=None, point_2d_uv=None, point_2d_norm=None, point_id=None, keypoints=None,
                    keypoints_norm=None):
        """-> dict(loop_index, connected, ids int32 [n], scores float64 [n]) of this frame's query and gates"""
        from .bow import RESULT_DTYPE

        def arr(a, dt, width):
            return np.zeros((0, width), dt) if a is None else np.ascontiguousarray(a, dt).reshape(-1, width)
        p3, uv, nm = arr(point_3d, np.float32, 3), arr(point_2d_uv, np.float32, 2), arr(point_2d_norm, np.float32, 2)
        ids = arr(point_id, np.float64, 1).reshape(-1)
        kp, kn = arr(keypoints, np.float32, 2), arr(keypoints_norm, np.float32, 2)
        if not len(p3) == len(uv) == len(nm) == len(ids) or len(kp) != len(kn):
            raise ValueError("the vectors of one group differ in length")
        out = (C.c_int32 * 3)()
        ret = np.zeros(4, RESULT_DTYPE)
        self._check(self.hl.dll.lvh_bow_add_keyframe(self._d, int(slot), int(index), 1 if flag_detect_loop else 0, len(uv), A._ptr(p3), A._ptr(uv), A._ptr(nm),
                                                     A._ptr(ids), len(kp), A._ptr(kp), A._ptr(kn), out, A._ptr(ret)), "lvh_bow_add_keyframe")
        return dict(loop_index=out[0], connected=bool(out[1]), ids=ret["entry_id"][:out[2]].copy(), scores=ret["score"][:out[2]].copy())

    def usePnP(self, pnp):
        """LoopDetector::usePnP: addKeyFrame's `connected` becomes the whole KeyFrame::findConnection (PnPRANSAC and the
        second > MIN_LOOP_NUM gate, keyframe.cpp:200-211) through this HostPnPRansac; None removes the hook"""
        if not self.hl.has_pnp:
            raise RuntimeError("this host library has no loop confirmation (only the one linked against liblvi_hip.so has)")
        code = self.hl.dll.lvh_bow_use_pnp(self._d, pnp._p if pnp is not None else None)
        if code < 0:
            raise A.LviError(code, "lvh_bow_use_pnp", self.hl.dll.lvh_pnp_last_error().decode(errors="replace"))
        self._pnp = pnp                                                  # keeps it alive while installed

    def pnp_connection(self):
        """matched_3d [n, 3], matched_2d_old_norm [n, 2] as PnPRANSAC received them in the last addKeyFrame and its
        status [n]; n == 0 when PnPRANSAC did not run (no hook, no loop, or the first gate failed)"""
        n = self.hl.dll.lvh_bow_pnp_connection(self._d, None, None, None)
        if n < 0:
            raise A.LviError(n, "lvh_bow_pnp_connection", self.hl.dll.lvh_pnp_last_error().decode(errors="replace"))
        p3 = np.zeros((max(n, 1), 3), np.float32); p2 = np.zeros((max(n, 1), 2), np.float32); st = np.zeros(max(n, 1), np.uint8)
        self.hl.dll.lvh_bow_pnp_connection(self._d, A._ptr(p3), A._ptr(p2), A._ptr(st))
        return p3[:n].copy(), p2[:n].copy(), st[:n].copy()

    def connection(self):
        """matched_2d_cur, matched_2d_old [n, 2] and matched_id [n] of the last hit's findConnectionFront (with usePnP:
        of findConnection, after PnPRANSAC's compaction)"""
        n = self._check(self.hl.dll.lvh_bow_connection(self._d, None, None, None), "lvh_bow_connection")
        cur = np.zeros((max(n, 1), 2), np.float32); old = np.zeros((max(n, 1), 2), np.float32); ids = np.zeros(max(n, 1), np.float64)
        self._check(self.hl.dll.lvh_bow_connection(self._d, A._ptr(cur), A._ptr(old), A._ptr(ids)), "lvh_bow_connection")
        return cur[:n].copy(), old[:n].copy(), ids[:n].copy()


class HostPnPRansac(_HostOwned):
    """lvi_host::PnPRansac (host/lvi_pnp_host.hpp): KeyFrame::PnPRANSAC (keyframe.cpp:135-176) with the reference's
    arguments (100 iterations, 10.0 / 460.0, 0.99).  HIP host library only.  Install it with LoopDetector.usePnP."""
    _ptr, _destroy, _last_error = "_p", "lvh_pnp_destroy", "lvh_pnp_last_error"

    def __init__(self, hostlib, device=0, max_points=2048, max_iters=100):
        if not hostlib.has_pnp:
            raise RuntimeError("this host library has no loop confirmation (only the one linked against liblvi_hip.so has)")
        self.hl = hostlib
        self._p = hostlib.dll.lvh_pnp_create(int(device), int(max_points), int(max_iters))
        if not self._p:
            raise A.LviError(-1, "lvh_pnp_create", hostlib.dll.lvh_pnp_last_error().decode(errors="replace"))

    def status(self, matched_2d_old_norm, matched_3d):
        """the status vector of keyframe.cpp:167-174"""
        p2 = np.ascontiguousarray(matched_2d_old_norm, np.float32).reshape(-1, 2)
        p3 = np.ascontiguousarray(matched_3d, np.float32).reshape(-1, 3)
        if len(p2) != len(p3):
            raise ValueError("the vectors differ in length")
        st = np.zeros(max(len(p2), 1), np.uint8)
        code = self.hl.dll.lvh_pnp_status(self._p, A._ptr(p2), A._ptr(p3), len(p2), A._ptr(st))
        if code < 0:
            raise A.LviError(code, "lvh_pnp_status", self.hl.dll.lvh_pnp_last_error().decode(errors="replace"))
        return st[:len(p2)].copy()


class PoseGraphBackend(_HostOwned):
    """lvi_host::PoseGraphBackend (host/lvi_pgo_host.hpp): mapOptimization's factor graph over include/lvi_pgo.h and
    include/lvi_pgo_gps.h (graph.add_gps, graph.gps_count, graph.marginal_covariance).  HIP host library only.  Install it with SequentialMapper.usePoseGraph and feed it what
    LoopCloser.pop() returns.  `graph` is a pgo.PoseGraph view of the handle the C++ side owns."""
    _ptr, _destroy, _last_error = "_p", "lvh_pgo_destroy", "lvh_pgo_last_error"

    def __init__(self, hostlib, abi_lib, device=0, max_poses=4096, max_loops=64, full_logmap=-1, max_iters=0, conv_eps=0.0):
        from .pgo import PgoParams, PoseGraph, bind as pgo_bind
        if not hostlib.has_pgo:
            raise RuntimeError("this host library has no pose-graph back end (only the one linked against liblvi_hip.so has)")
        self.hl = hostlib
        self._p = hostlib.dll.lvh_pgo_create(int(device), int(max_poses), int(max_loops), int(full_logmap), int(max_iters), float(conv_eps))
        if not self._p:
            raise A.LviError(-1, "lvh_pgo_create", hostlib.dll.lvh_pgo_last_error().decode(errors="replace"))
        self.graph = PoseGraph.__new__(PoseGraph)                         # never destroyed from here
        self.graph.lib = pgo_bind(abi_lib)
        self.graph.max_poses, self.graph.max_loops = int(max_poses), int(max_loops)
        self.graph._h = C.c_void_p(hostlib.dll.lvh_pgo_handle(self._p))
        self.graph.params = PgoParams()
        self.graph.close = lambda: None

    def push_loop(self, constraint):
        """a dict of LoopCloser.pop(): key_cur, key_pre, between [4, 4], noise; returns the queue's length"""
        b = np.ascontiguousarray(constraint["between"], np.float64).reshape(16)
        n = self.hl.dll.lvh_pgo_push_loop(self._p, int(constraint["key_cur"]), int(constraint["key_pre"]), b.ctypes.data_as(C.POINTER(C.c_double)),
                                          float(constraint["noise"]))
        if n < 0:
            raise A.LviError(n, "lvh_pgo_push_loop", self.hl.dll.lvh_pgo_last_error().decode(errors="replace"))
        return n

    def add_gps(self, key, xyz, variance):
        """GPSFactor(key, xyz, Variances(variance)) on the graph the C++ side owns (include/lvi_pgo_gps.h); the node's GpsGate adds
        its own through MapOptimizationNode::useGps"""
        self.graph.add_gps(key, xyz, variance)

    def gps_count(self):
        return self.graph.gps_count()

    def marginal_covariance(self, key):
        """isam->marginalCovariance(key) (mapOptimization.cpp:1591) -> [6, 6] float64"""
        return self.graph.marginal_covariance(key)

    def last(self):
        """dict(updates, loops_added, loops_queued, status, info of the last update, pose_to of the last addOdomFactor)"""
        from .pgo import PgoInfo
        info, pose, cnt = PgoInfo(), (C.c_float * 6)(), (C.c_int32 * 4)()
        self.hl.dll.lvh_pgo_last(self._p, C.byref(info), pose, cnt)
        return dict(updates=cnt[0], loops_added=cnt[1], loops_queued=cnt[2], status=cnt[3], iterations=info.iterations, converged=bool(info.converged),
                    chi2_before=info.chi2_before, chi2_after=info.chi2_after, max_step=info.max_step, pose_to=np.array(pose[:], np.float32))


class VinsMarginalizer(_HostOwned):
    """lvi_host::VinsMarginalizer (host/lvi_marg_host.hpp): the MARGIN_OLD and MARGIN_SECOND_NEW branches of
    Estimator::optimization (estimator.cpp:813-976) over include/lvi_marg.h, the prior resident on the device.  HIP host
    library only.  `marg` is a marg.Marginalizer view of the handle the C++ side owns (layout, prior, debug_system)."""
    _ptr, _destroy, _last_error = "_p", "lvh_marg_destroy", "lvh_marg_last_error"
    MARGIN_OLD, MARGIN_SECOND_NEW = 0, 1
    WINDOW_SIZE = 10

    def __init__(self, hostlib, abi_lib, device=0, max_features=150, estimate_td=True, **params):
        from .marg import Marginalizer, MargParams, bind as marg_bind
        if not hostlib.has_marg:
            raise RuntimeError("this host library has no marginalisation (only the one linked against liblvi_hip.so has)")
        self.hl = hostlib
        p = MargParams()
        marg_bind(abi_lib).dll.lvi_marg_params_default(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise AttributeError(f"lvi_marg_params has no field {k}")
            setattr(p, k, v)
        self._p = hostlib.dll.lvh_marg_create(int(device), int(max_features), int(bool(estimate_td)), C.byref(p))
        if not self._p:
            raise A.LviError(-1, "lvh_marg_create", hostlib.dll.lvh_marg_last_error().decode(errors="replace"))
        self.marg = Marginalizer(abi_lib, handle=hostlib.dll.lvh_marg_handle(self._p))       # never destroyed from here
        self.marg.params = p

    def close(self):
        super().close()
        self.marg._h = C.c_void_p()                  # the view's handle went with the C++ object

    def set_window(self, pose, speed_bias, ex_pose, td):
        """vector2double: para_Pose [11, 7], para_SpeedBias [11, 9], para_Ex_Pose [7], para_Td"""
        dp = C.POINTER(C.c_double)
        a, b, c = (np.ascontiguousarray(x, np.float64) for x in (pose, speed_bias, ex_pose))
        assert a.shape == (self.WINDOW_SIZE + 1, 7) and b.shape == (self.WINDOW_SIZE + 1, 9) and c.shape == (7,)
        self._check(self.hl.dll.lvh_marg_set_window(self._p, a.ctypes.data_as(dp), b.ctypes.data_as(dp), c.ctypes.data_as(dp), float(td)), "lvh_marg_set_window")

    def set_features(self, features):
        """f_manager.feature: dicts of start_frame, inv_dep and obs (dicts of point [3], velocity [2], cur_td, uv_y)"""
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        start = np.array([f["start_frame"] for f in features], np.int32)
        n_obs = np.array([len(f["obs"]) for f in features], np.int32)
        inv = np.array([f["inv_dep"] for f in features], np.float64)
        obs = np.array([[*o["point"], *o["velocity"], o["cur_td"], o["uv_y"]] for f in features for o in f["obs"]], np.float64).reshape(-1, 7)
        self._check(self.hl.dll.lvh_marg_set_features(self._p, len(features), start.ctypes.data_as(ip), n_obs.ctypes.data_as(ip), inv.ctypes.data_as(dp),
                                                      obs.ctypes.data_as(dp)), "lvh_marg_set_features")

    def set_imu(self, sum_dt, residual=None, jacobians=None):
        """pre_integrations[1]->sum_dt and IMUFactor evaluated by the caller: residual [15], jacobians [15, 7], [15, 9], [15, 7], [15, 9]"""
        dp = C.POINTER(C.c_double)
        if residual is None:
            return self._check(self.hl.dll.lvh_marg_set_imu(self._p, float(sum_dt), None, None), "lvh_marg_set_imu")
        r = np.ascontiguousarray(residual, np.float64).reshape(15)
        J = np.concatenate([np.ascontiguousarray(j, np.float64).reshape(15, s).ravel() for j, s in zip(jacobians, (7, 9, 7, 9))])
        return self._check(self.hl.dll.lvh_marg_set_imu(self._p, float(sum_dt), r.ctypes.data_as(dp), J.ctypes.data_as(dp)), "lvh_marg_set_imu")

    def run(self, flag):
        """one pass through estimator.cpp:813-976 -> dict(ran, status, m, n, rank, ...)"""
        from .marg import MargInfo
        info, ran = MargInfo(), C.c_int32(0)
        st = self._check(self.hl.dll.lvh_marg_run(self._p, int(flag), C.byref(ran), C.byref(info)), "lvh_marg_run")
        return dict(ran=bool(ran.value), status=st, **{k: getattr(info, k) for k, _ in MargInfo._fields_})


class VinsWindowOptimizer(_HostOwned):
    """lvi_host::VinsWindowOptimizer (host/lvi_win_host.hpp): the first half of Estimator::optimization (estimator.cpp:696-811)
    over include/lvi_win.h, on the window arrays of a VinsMarginalizer and with its resident prior: `optimize(flag)` then
    `marginalizer.run(flag)` is the tail of Estimator::optimization with no prior on the bus.  HIP host library only."""
    _ptr, _destroy, _last_error = "_p", "lvh_win_destroy", "lvh_win_last_error"

    def __init__(self, hostlib, abi_lib, marginalizer, device=0, max_features=150, estimate_extrinsic=0, num_iterations=8, solver_time=0.0, **params):
        from .win import WinParams, bind as win_bind
        if not hostlib.has_win:
            raise RuntimeError("this host library has no window solve (only the one linked against liblvi_hip.so has)")
        self.hl, self.vm = hostlib, marginalizer
        p = WinParams()
        win_bind(abi_lib).dll.lvi_win_params_default(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise AttributeError(f"lvi_win_params has no field {k}")
            setattr(p, k, (C.c_double * 3)(*v) if k == "G" else v)
        self._p = hostlib.dll.lvh_win_create(marginalizer._p, int(device), int(max_features), int(estimate_extrinsic), int(num_iterations), float(solver_time),
                                             C.byref(p))
        if not self._p:
            raise A.LviError(-1, "lvh_win_create", hostlib.dll.lvh_win_last_error().decode(errors="replace"))

    def set_imu(self, j, record=None):
        """pre_integrations[j], j = 1..WINDOW_SIZE: a one-element win.IMU_DTYPE array (its ids are ignored), or None for no factor"""
        from .win import IMU_DTYPE
        if record is None:
            return self._check(self.hl.dll.lvh_win_set_imu(self._p, int(j), None), "lvh_win_set_imu")
        r = np.ascontiguousarray(record, IMU_DTYPE).reshape(1)
        return self._check(self.hl.dll.lvh_win_set_imu(self._p, int(j), r.ctypes.data_as(C.c_void_p)), "lvh_win_set_imu")

    def set_lidar_flags(self, flags):
        f = np.ascontiguousarray(flags, np.int32)
        self._check(self.hl.dll.lvh_win_set_lidar_flags(self._p, len(f), f.ctypes.data_as(C.POINTER(C.c_int32))), "lvh_win_set_lidar_flags")

    def optimize(self, flag):
        """estimator.cpp:696-811 -> dict(status, iterations, termination, initial_cost, final_cost, ...)"""
        from .win import WinInfo
        info = WinInfo()
        st = self._check(self.hl.dll.lvh_win_optimize(self._p, int(flag), C.byref(info)), "lvh_win_optimize")
        return dict(status=st, **{k: getattr(info, k) for k, _ in WinInfo._fields_})

    def window(self):
        """-> dict(pose [11, 7], speed_bias [11, 9], ex_pose [7], td, inv_dep [features]): what double2vector reads"""
        dp = C.POINTER(C.c_double)
        n = C.c_int32(0)
        self._check(self.hl.dll.lvh_win_get_window(self._p, None, None, None, None, 0, C.byref(n), None), "lvh_win_get_window")
        pose, sb, ex, td, inv = np.zeros((11, 7)), np.zeros((11, 9)), np.zeros(7), C.c_double(0), np.zeros(max(1, n.value))
        self._check(self.hl.dll.lvh_win_get_window(self._p, pose.ctypes.data_as(dp), sb.ctypes.data_as(dp), ex.ctypes.data_as(dp), C.byref(td), n.value, None,
                                                   inv.ctypes.data_as(dp)), "lvh_win_get_window")
        return dict(pose=pose, speed_bias=sb, ex_pose=ex, td=td.value, inv_dep=inv[:n.value])


class FeatureManager(_HostOwned):
    """lvi_host::FeatureManager (host/lvi_fman_host.hpp): the reference's f_manager over include/lvi_fman.h, with fillWindow /
    takeDepths towards a VinsMarginalizer and a VinsWindowOptimizer and the two slides of estimator.cpp:1076-1099.  HIP host
    library only.  `table` is a fman.FeatureTable view of the handle the C++ side owns (download, projections, ...)."""
    _ptr, _destroy, _last_error = "_p", "lvh_fman_destroy", "lvh_fman_last_error"

    def __init__(self, hostlib, abi_lib, device=0, max_features=1024, **params):
        from .fman import FeatureTable, FmanParams, bind as fman_bind
        if not hostlib.has_fman:
            raise RuntimeError("this host library has no feature manager (only the one linked against liblvi_hip.so has)")
        self.hl = hostlib
        p = FmanParams()
        fman_bind(abi_lib).dll.lvi_fman_params_default(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise AttributeError(f"lvi_fman_params has no field {k}")
            setattr(p, k, v)
        self._p = hostlib.dll.lvh_fman_create(int(device), int(max_features), C.byref(p))
        if not self._p:
            raise A.LviError(-1, "lvh_fman_create", hostlib.dll.lvh_fman_last_error().decode(errors="replace"))
        self.table = FeatureTable(abi_lib, max_features=max_features, handle=hostlib.dll.lvh_fman_handle(self._p))    # never destroyed from here
        self.table.params = p

    def close(self):
        super().close()
        self.table._h = C.c_void_p()                  # the view's handle went with the C++ object

    def clear_state(self):
        self._check(self.hl.dll.lvh_fman_clear_state(self._p), "lvh_fman_clear_state")

    def add_frame(self, frame_count, ids, obs, td=0.0):
        """addFeatureCheckParallax -> dict(last_track_num, parallax_num, keyframe, added, parallax_sum)"""
        from .fman import FmanFrameInfo
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 8)
        assert len(obs) == len(ids)
        info = FmanFrameInfo()
        key = self._check(self.hl.dll.lvh_fman_add_frame(self._p, int(frame_count), len(ids), ids.ctypes.data_as(ip), obs.ctypes.data_as(dp), float(td),
                                                         C.byref(info)), "lvh_fman_add_frame")
        out = {k: getattr(info, k) for k, _ in FmanFrameInfo._fields_}
        assert out["keyframe"] == key
        return out

    def triangulate(self, Ps, Rs, tic, ric):
        from .fman import FmanTriInfo
        dp = C.POINTER(C.c_double)
        a, b, c, d = (np.ascontiguousarray(x, np.float64) for x in (Ps, Rs, tic, ric))
        assert a.shape == (11, 3) and b.shape == (11, 3, 3) and c.shape == (3,) and d.shape == (3, 3)
        info = FmanTriInfo()
        self._check(self.hl.dll.lvh_fman_triangulate(self._p, a.ctypes.data_as(dp), b.ctypes.data_as(dp), c.ctypes.data_as(dp), d.ctypes.data_as(dp),
                                                     C.byref(info)), "lvh_fman_triangulate")
        return {k: getattr(info, k) for k, _ in FmanTriInfo._fields_}

    def fill_window(self, marginalizer, optimizer):
        """fillWindow: `features` and `lidarDepthFlag` of a VinsMarginalizer / VinsWindowOptimizer pair from the table"""
        self._check(self.hl.dll.lvh_fman_fill_window(self._p, marginalizer._p, optimizer._p), "lvh_fman_fill_window")

    def take_depths(self, marginalizer):
        """takeDepths: setDepth with the inverse depths the window solve left"""
        self._check(self.hl.dll.lvh_fman_take_depths(self._p, marginalizer._p), "lvh_fman_take_depths")

    def remove_failures(self):
        self._check(self.hl.dll.lvh_fman_remove_failures(self._p), "lvh_fman_remove_failures")

    def slide_old(self, shift_depth, back_R0=None, back_P0=None, Rs0=None, Ps0=None, ric=None, tic=None):
        """slideWindowOld (estimator.cpp:1082-1099)"""
        dp = C.POINTER(C.c_double)
        if not shift_depth:
            return self._check(self.hl.dll.lvh_fman_slide_old(self._p, 0, None, None, None, None, None, None), "lvh_fman_slide_old")
        arrs = [np.ascontiguousarray(x, np.float64) for x in (back_R0, back_P0, Rs0, Ps0, ric, tic)]
        assert [x.size for x in arrs] == [9, 3, 9, 3, 9, 3]
        return self._check(self.hl.dll.lvh_fman_slide_old(self._p, 1, *[x.ctypes.data_as(dp) for x in arrs]), "lvh_fman_slide_old")

    def slide_new(self, frame_count=10):
        """slideWindowNew (estimator.cpp:1076-1080)"""
        self._check(self.hl.dll.lvh_fman_slide_new(self._p, int(frame_count)), "lvh_fman_slide_new")


class TrackerRig(_HostOwned):
    """FeatureTrackerRig of host/lvi_tbatch_host.hpp: FeatureTracker::readImage for S cameras over one batch tracker handle
    (include/lvi_tbatch.h), and the node's updateID loop (feature_tracker_node.cpp:136-166).  The reference compiles
    NUM_OF_CAM = 1: a capability of the library, not a restated behaviour.  ``batched=False`` is the yardstick: one
    FeatureTracker over one lvi_tracker per camera, called one after another.  HIP host library only."""
    _ptr, _destroy, _last_error = "_r", "lvh_rig_destroy", "lvh_rig_last_error"

    def __init__(self, hostlib, tracker_params, slots, row, col, equalize=False, cams=None, device=0, batched=True):
        if not hostlib.has_rig:
            raise RuntimeError("this host library has no camera rig (only the one linked against liblvi_hip.so has)")
        self.hl = hostlib
        self.slots = int(slots)
        tab = None
        if cams is not None:
            if len(cams) != self.slots:
                raise ValueError("one camera model per slot")
            tab = (A.MeiParams * self.slots)(*[A.MeiParams(*[float(c[k]) for k in ("xi", "k1", "k2", "p1", "p2", "gamma1", "gamma2", "u0", "v0")]) for c in cams])
        self._r = hostlib.dll.lvh_rig_create(C.byref(tracker_params), self.slots, int(device), int(row), int(col), 1 if equalize else 0, tab, 1 if batched else 0)
        if not self._r:
            raise A.LviError(-3, "lvh_rig_create", hostlib.dll.lvh_rig_last_error().decode(errors="replace"))
        self.cap = int(tracker_params.max_features)

    def use_device_fundamental(self, device=0):
        """every camera's rejectWithF runs the device RANSAC (include/lvi_fmat.h) through a handle of its own"""
        self._check(self.hl.dll.lvh_rig_use_device_fundamental(self._r, int(device)), "lvh_rig_use_device_fundamental")

    def use_batched_fundamental(self, device=0):
        """rejectWithF of all cameras runs as ONE call of the batched device RANSAC per frame (include/lvi_fmatb.h); the
        batched rig only (LVI_ERR_STATE otherwise)"""
        self._check(self.hl.dll.lvh_rig_use_batched_fundamental(self._r, int(device)), "lvh_rig_use_batched_fundamental")

    def fundamental_stats(self):
        """dict(rejectWithF_skipped, rejectWithF_removed: summed over the cameras; calls: findFundamentalMat calls made (the
        batched handle's, or the per-camera device hooks'); prepared: cameras that prepared over all frames (batched only))"""
        out = (C.c_int64 * 4)()
        self._check(self.hl.dll.lvh_rig_fundamental_stats(self._r, out), "lvh_rig_fundamental_stats")
        return dict(rejectWithF_skipped=int(out[0]), rejectWithF_removed=int(out[1]), calls=int(out[2]), prepared=int(out[3]))

    def reset_ids(self):
        """FeatureTracker::n_id := 0 (one counter per process)"""
        self.hl.dll.lvh_rig_reset_ids()

    def read_images(self, imgs, times, pub_this_frame):
        """imgs: one row x col uint8 image per camera (None: no image for that camera this frame)"""
        arrs = [None if x is None else np.ascontiguousarray(x, np.uint8) for x in imgs]
        ptrs = (C.c_void_p * self.slots)(*[A._ptr(a) if a is not None else None for a in arrs])
        t = (C.c_double * self.slots)(*[float(v) for v in times])
        pub = (C.c_int32 * self.slots)(*[1 if v else 0 for v in pub_this_frame])
        self._check(self.hl.dll.lvh_rig_read_images(self._r, ptrs, t, pub), "lvh_rig_read_images")

    def update_ids(self):
        self._check(self.hl.dll.lvh_rig_update_ids(self._r), "lvh_rig_update_ids")

    def camera(self, cam):
        """dict(cur_pts, cur_un_pts, pts_velocity [n,2] f32; ids, track_cnt [n] i32) of one camera after the last frame"""
        n = C.c_int32(0)
        rows = np.zeros((self.cap, 6), np.float32)
        ic = np.zeros((self.cap, 2), np.int32)
        self._check(self.hl.dll.lvh_rig_camera(self._r, int(cam), A._ptr(rows), A._ptr(ic), self.cap, C.byref(n)), "lvh_rig_camera")
        m = n.value
        return dict(cur_pts=rows[:m, 0:2].copy(), cur_un_pts=rows[:m, 2:4].copy(), pts_velocity=rows[:m, 4:6].copy(), ids=ic[:m, 0].copy(), track_cnt=ic[:m, 1].copy())
