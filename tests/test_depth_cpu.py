"""CPU tier: the LiDAR depth association's interface (include/lvi_depth.h, its binding, the host library that carries its
flattening) and known-answer tests of its restatement (tests/depth_ref.py)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import depth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "lvi_depth.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lvi_depth_[a-z0-9_]+)\s*\(", txt)))


def test_header_and_depth_binding_agree(pkg):
    assert _declared() == sorted(pkg.depth.DEPTH_SIGNATURES.keys())
    assert not set(_declared()) & set(pkg._abi.SIGNATURES), "the depth ABI must stay out of lvi_hotpath.h's table"


def test_hip_library_exports_the_depth_abi(pkg):
    dll = ctypes.CDLL(pkg.HIP_LIB_PATH)
    for name in _declared():
        assert hasattr(dll, name), f"{name} missing from liblvi_hip.so"
    lib = pkg.depth.bind(pkg.load_hip())
    assert lib.dll.lvi_depth_abi_version() == 1
    assert lib.dll.lvi_abi_version() == 6


def test_depth_register_fails_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.LviError) as e:
        pkg.DepthRegister(pkg.load_hip())
    assert e.value.code == pkg._abi.LVI_ERR_NO_DEVICE


def test_host_libraries_link(pkg, oracle, tmp_path):
    """the oracle-linked host library builds without the depth flattening; the HIP one carries it"""
    H = pkg.host_api
    out = tmp_path / "liblvi_host_oracle.so"
    H.build_host_library(str(out), os.path.dirname(oracle.path), "lvi_oracle", extra=("-fopenmp",))
    hl = H.HostLibrary(str(out))
    assert not hl.has_depth
    assert os.path.exists(H.HOST_HIP_LIB), "host/liblvi_host_hip.so not built: run __graft_entry__.build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", H.HOST_HIP_LIB], capture_output=True, text=True).stdout
    for s in ("lvh_depth_create", "lvh_depth_install", "lvh_depth_lidar", "lvh_depth_set_image_pose", "lvh_trk_image"):
        assert s in syms, s


def test_camera_yaml_lidar_settings(pkg):
    s = pkg.config.load_camera_lidar_yaml(os.path.join(ROOT, "tests", "golden", "params_camera.yaml"))
    assert s == dict(use_lidar=1, lidar_skip=3, point_cloud_topic="/lio_sam/deskew/cloud_deskewed")


# ---------------------------------------------------------------------------------------------- restatement KATs
IDENT = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def _plane_cloud(x0, half=4.0, step=0.05):
    """a wall x = x0 in front of the body, about one point per step x step"""
    n = int(round(2 * half / step)) ** 2
    rng = np.random.default_rng(int(x0 * 1000) + n)           # scattered: three grid neighbours would be collinear (s = 0 / 0)
    yz = rng.uniform(-half, half, (n, 2)).astype(np.float32)
    return np.stack([np.full(n, x0, np.float32), yz[:, 0], yz[:, 1], np.ones(n, np.float32)], 1)


def test_inverse_is_eigen_order(oracle):
    pose = (1.5, -2.0, 0.3, 0.1, -0.2, 0.7)
    M = R.get_transformation(oracle, pose)
    Mi = R.affine_inverse(M)
    I = Mi[:, :3].astype(np.float64) @ M[:, :3].astype(np.float64)
    assert np.abs(I - np.eye(3)).max() < 1e-6
    t = Mi[:, :3].astype(np.float64) @ M[:, 3] + Mi[:, 3]
    assert np.abs(t).max() < 1e-5


def test_plane_gives_the_analytic_depth(oracle):
    cloud = _plane_cloud(10.0)
    feats = np.array([[0.0, 0.0, 1.0], [0.05, -0.03, 1.0], [-0.1, 0.08, 1.0]], np.float32)
    d, dbg = R.get_depth(oracle, cloud, IDENT, feats)
    # a feature (u, v, 1) meets the wall x = 10 at camera depth z = 10: the published value is the body-x of the hit
    assert np.all(np.abs(d - 10.0) < 1e-3), d
    assert len(dbg["sphere"]) >= 10


def test_fewer_than_ten_points_give_minus_one(oracle):
    y = np.linspace(-2.0, 2.0, 9, dtype=np.float32)                 # nine points, nine bins
    cloud = np.stack([np.full(9, 10.0, np.float32), y, np.zeros(9, np.float32), np.ones(9, np.float32)], 1)
    d, dbg = R.get_depth(oracle, cloud, IDENT, [[0, 0, 1]])
    assert len(dbg["sphere"]) == 9 and (d == -1).all() and "nbr" not in dbg


def _sphere(pts):
    """body-frame points -> unit-sphere entries as step 5 makes them"""
    p = np.array([[*q, 1.0] for q in pts], np.float32)
    sph, _ = R.sphere_cloud(p, np.arange(len(p)).reshape(1, -1))
    return sph


AXIS = R.feature_rays([[0, 0, 1]])[0]                               # the optical axis = body x


def test_depth_spread_and_small_s_give_minus_one():
    sph = _sphere([(10.0, 0.02, 0.02), (10.0, -0.02, 0.02), (13.0, 0.0, -0.03)])
    assert R.intersect(sph, [0, 1, 2], AXIS) == -1                  # max - min > 2
    sph = _sphere([(10.0, 0.02, 0.02), (10.0, -0.02, 0.02), (11.9, 0.0, -0.03)])
    assert R.intersect(sph, [0, 1, 2], AXIS) > 3                    # within the spread
    sph = _sphere([(0.4, 0.01, 0.0), (0.4, -0.01, 0.01), (0.4, 0.0, -0.01)])
    assert R.intersect(sph, [0, 1, 2], AXIS) == -1                  # s = 0.4 <= 0.5


def test_clamp_at_min_and_max():
    # plane x = 10 + 50 (y - 0.01): meets the axis at 9.5 < min -> clamped to the smallest range
    sph = _sphere([(10.0, 0.01, 0.01), (10.5, 0.02, 0.01), (10.0, 0.01, 0.02)])
    assert R.intersect(sph, [0, 1, 2], AXIS) == np.float32(AXIS[0] * sph[:, 3].min())
    # plane x = 10 - 50 (y - 0.01): meets the axis at 10.5 > max -> clamped to the largest range
    sph = _sphere([(10.0, 0.01, 0.01), (9.5, 0.02, 0.01), (10.0, 0.01, 0.02)])
    assert R.intersect(sph, [0, 1, 2], AXIS) == np.float32(AXIS[0] * sph[:, 3].max())
    # inside [min, max]: the plane's own intersection
    sph = _sphere([(10.0, 0.01, 0.01), (10.0, -0.01, 0.01), (10.0, 0.0, -0.01)])
    assert abs(R.intersect(sph, [0, 1, 2], AXIS) - 10.0) < 1e-4


def test_depth_at_most_three_gives_minus_one(oracle):
    d, _ = R.get_depth(oracle, _plane_cloud(2.5, half=1.0, step=0.02), IDENT, [[0, 0, 1]])
    assert d[0] == -1
    d, _ = R.get_depth(oracle, _plane_cloud(3.2, half=1.0, step=0.02), IDENT, [[0, 0, 1]])
    assert abs(d[0] - 3.2) < 1e-4


def test_origin_point_passes_get_depths_test_but_not_the_callbacks(oracle):
    p = np.array([[0.0, 0.0, 0.0, 1.0]], np.float32)
    assert not R.fov_keep(p)[0]                                   # lidar_callback drops it (NaN ratios fail <=)
    sel = R.range_image(p)                                        # get_depth keeps it (NaN ratios fail >)
    assert sel[180, 0] == 0 and (sel >= 0).sum() == 1
    sph, _ = R.sphere_cloud(p, sel)
    assert np.isnan(sph[0, :3]).all() and sph[0, 3] == 0          # 0 / 0 on the sphere, counted among the points
    # x = 0, z != 0: |z / x| = inf > 10, skipped
    assert (R.range_image(np.array([[0.0, 0.0, 1.0, 1.0]], np.float32)) < 0).all()


def test_skip_counting_and_window_pop(pkg, oracle):
    W = R.Window(pkg, oracle, lidar_skip=2, window_s=5.0)
    cloud = _plane_cloud(8.0, half=2.0, step=0.3)
    used = [W.lidar_callback(cloud, IDENT, 0.5 * k) for k in range(13)]
    assert used == [k % 3 == 0 for k in range(13)]               # the first cloud is used, then every (LIDAR_SKIP + 1)-th
    assert W.stamps == [1.5, 3.0, 4.5, 6.0]                       # 6.0 - 0.0 > 5.0 popped; 6.0 - 1.5 = 4.5 kept
    assert not W.lidar_callback(cloud, IDENT, 6.5) and not W.lidar_callback(cloud, IDENT, 7.0)
    assert not W.lidar_callback(cloud, None, 7.5)                 # no TF: counted, nothing else
    assert W.lidar_count == 15 and W.stamps == [1.5, 3.0, 4.5, 6.0]
    assert not W.lidar_callback(cloud, IDENT, 8.0) and not W.lidar_callback(cloud, IDENT, 8.5)
    assert W.lidar_callback(cloud, IDENT, 11.0)                   # 11.0 - 6.0 = 5.0 is not > 5.0: 6.0 stays
    assert W.stamps == [6.0, 11.0]
    assert len(W.depth_cloud) > 0 and W.counts.sum() == 2 * len(W.voxel(cloud)[R.fov_keep(W.voxel(cloud))])


def test_threshold_and_band_constants():
    assert R.DIST_SQ_THRESHOLD == np.float32((math.sin(0.5 / 180.0 * math.pi) * 5.0) ** 2)
    arc = 2 * math.degrees(math.asin(math.sqrt(float(R.DIST_SQ_THRESHOLD)) / 2))
    assert arc / 0.5 + 0.5 < 7                                   # the kernel's band half-width (BAND_ROWS)
