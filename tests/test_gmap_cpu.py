"""CPU tier of the global map (include/lvi_gmap.h, host/lvi_gmap_host.hpp): the PCD writer byte for byte, publishGlobalMap's
key-selection restatement (gmap_ref.select_keys) on hand cases, and the exports of the two HIP-side libraries."""
import ctypes as C
import os
import subprocess
import textwrap

import numpy as np
import pytest

import gmap_ref as G

F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "lidar-visual-inertial-slam_amd")


def _exports(path):
    r = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
    return {line.split()[-1] for line in r.stdout.splitlines() if line.strip()}


def test_hip_library_exports_gmap(pkg):
    syms = _exports(pkg.HIP_LIB_PATH)
    for name in pkg.gmap.GMAP_SIGNATURES:
        assert name in syms, name
    with open(os.path.join(REPO, "include", "lvi_hotpath.h")) as f:
        assert "lvi_gmap" not in f.read()                     # a separate ABI: lvi_hotpath.h (and the oracle) untouched


def test_host_library_links_gmap(pkg):
    syms = _exports(pkg.host_api.HOST_HIP_LIB)
    for name in ("lvh_gmap_create", "lvh_gmap_reserve", "lvh_gmap_keys", "lvh_gmap_publish", "lvh_gmap_cloud", "lvh_gmap_save"):
        assert name in syms, name
    assert "lvh_gmap_create" not in _exports(pkg.HIP_LIB_PATH)


def test_pcd_writer_round_trip(tmp_path):
    """the binary PCD files of save_map: PCL's header byte for byte, the non-padding fields packed (16 B / 36 B per point)"""
    src = tmp_path / "w.cpp"
    src.write_text(textwrap.dedent("""
        #include "lvi_gmap_host.hpp"
        using namespace lvi_host;
        extern "C" int write_xyzi(const char* p, const lvi_pt* pts, int n) { return savePCDBinaryXYZI(p, std::vector<lvi_pt>(pts, pts + n)) ? 1 : 0; }
        extern "C" int write_pose(const char* p, const float* f, const double* t, int n)
        {
            std::vector<PointTypePose> v(n);
            for (int i = 0; i < n; i++) v[i] = PointTypePose{f[7 * i], f[7 * i + 1], f[7 * i + 2], f[7 * i + 3], f[7 * i + 4], f[7 * i + 5], f[7 * i + 6], t[i]};
            return savePCDBinaryPose6D(p, v) ? 1 : 0;
        }
        """))
    so = tmp_path / "libw.so"
    # declarations only from the product headers: nothing of the HIP library is called, so nothing is linked
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-I", os.path.join(PKG, "host"), str(src), "-o", str(so),
                    "-Wl,--unresolved-symbols=ignore-all"], check=True)
    lib = C.CDLL(str(so))
    rng = np.random.default_rng(3)
    pts = rng.normal(0, 50, (37, 4)).astype(F32)
    assert lib.write_xyzi(str(tmp_path / "a.pcd").encode(), pts.ctypes.data_as(C.c_void_p), len(pts)) == 1
    data = (tmp_path / "a.pcd").read_bytes()
    hdr = (b"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\n"
           b"COUNT 1 1 1 1\nWIDTH 37\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 37\nDATA binary\n")
    assert data[:len(hdr)] == hdr and len(data) == len(hdr) + 16 * 37
    np.testing.assert_array_equal(np.frombuffer(data[len(hdr):], np.uint32), pts.view(np.uint32).reshape(-1))
    f = rng.normal(0, 3, (5, 7)).astype(F32)
    t = rng.uniform(1e9, 2e9, 5)
    assert lib.write_pose(str(tmp_path / "b.pcd").encode(), f.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), 5) == 1
    data = (tmp_path / "b.pcd").read_bytes()
    hdr = (b"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity roll pitch yaw time\n"
           b"SIZE 4 4 4 4 4 4 4 8\nTYPE F F F F F F F F\nCOUNT 1 1 1 1 1 1 1 1\nWIDTH 5\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 5\nDATA binary\n")
    assert data[:len(hdr)] == hdr and len(data) == len(hdr) + 36 * 5
    rec = np.frombuffer(data[len(hdr):], np.dtype([("f", "<f4", 7), ("t", "<f8")]))
    np.testing.assert_array_equal(rec["f"].view(np.uint32), f.view(np.uint32))
    np.testing.assert_array_equal(rec["t"].view(np.uint64), t.view(np.uint64))


@pytest.fixture(scope="module")
def vf(pkg, oracle):
    o = pkg.LidarHotpath(oracle, N_SCAN=4, Horizon_SCAN=1024, max_raw_points=4096, max_map_points=4096)

    def f(pts, leaf):
        p = np.ascontiguousarray(pts, F32).reshape(-1, 4)
        return np.ascontiguousarray(o.voxel_downsample(p.view(pkg.PT_DTYPE).reshape(-1), float(leaf))).view(F32).reshape(-1, 4)
    yield f
    o.close()


def _poses(xyz):
    p = np.zeros((len(xyz), 4), F32)
    p[:, :3] = np.asarray(xyz, F32)
    p[:, 3] = np.arange(len(xyz))
    return p


def test_select_distance_ties(vf):
    """four keys at the same distance from back(): every one kept once, in VoxelGrid order (z, y, x), not search order"""
    p = _poses([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 0)])
    np.testing.assert_array_equal(G.select_keys(p, 1000.0, 0.1, vf), [3, 1, 4, 0, 2])
    # the nearest key of a DS centroid equidistant from two keys: the first index
    p = _poses([(0.25, 0, 0), (0.75, 0, 0), (5.5, 0, 0)])
    np.testing.assert_array_equal(G.select_keys(p, 1000.0, 1.0, vf), [0, 2])


def test_select_two_ds_poses_one_key(vf):
    """the centroid of voxel (0,0,0) is nearer to the key of voxel (1,0,0) than to its own keys: that key is fused twice"""
    p = _poses([(0.0, 0.0, 0.0), (0.9, 0.9, 0.0), (1.0, 0.45, 0.0)])
    np.testing.assert_array_equal(G.select_keys(p, 1000.0, 1.0, vf), [2, 2])


def test_select_radius(vf):
    """keys beyond R of back() are not searched; the DS centroid, not a key, is what the radius test (pointDistance) and the
    nearest-key lookup see"""
    p = _poses([(0.5, 0.5, 0.5), (30.0, 0, 0), (9.5, 0, 0), (10.5, 0, 0), (0, 0, 0)])
    # R = 10: key 1 (30 m) and key 3 (10.5 m) are outside; key 2 at 9.5 m is kept; VoxelGrid order (z, y, x)
    np.testing.assert_array_equal(G.select_keys(p, 10.0, 0.5, vf), [4, 2, 0])
    # one 20 m voxel holds keys 0, 2, 4 (3 is outside R): centroid (10/3, 1/6, 1/6) -> nearest key 0, one entry
    np.testing.assert_array_equal(G.select_keys(p, 10.0, 20.0, vf), [0])
