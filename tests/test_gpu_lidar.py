"""GPU tier (-m gpu): the HIP lidar path against the CPU oracle through the same C-ABI.

Bar (BASELINE.json north_star): point indices / voxel keys / column indices bit-exact;
f32 values that follow a fixed operation order bit-exact; voxel centroids within
count * 2^-23 * max|coord| (PCL's sum order inside a voxel is unspecified); pose within
1e-4 m / 1e-4 rad.  PARITY UNPINNED: the oracle restates the reference, which ships no
golden vectors (see oracle/ headers)."""
import ctypes

import numpy as np
import pytest

import centroid_ref
from helpers import bits, centroid_tol, make_small_scene, small_params, xyzi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(pkg, oracle):
    return make_small_scene(pkg, oracle)


@pytest.fixture(params=[1, 2], ids=["vox_sorted", "vox_binned"])
def pair(request, pkg, oracle, hip):
    """every test that takes `pair` runs once per realisation of the voxel grids (lvi_lidar_params.voxel_mode)"""
    o = pkg.LidarHotpath(oracle, **small_params())
    g = pkg.LidarHotpath(hip, voxel_mode=request.param, **small_params())
    yield o, g
    o.close(); g.close()


def _assert_info_equal(a, b):
    assert a["n"] == b["n"]
    np.testing.assert_array_equal(a["start_ring_index"], b["start_ring_index"])
    np.testing.assert_array_equal(a["end_ring_index"], b["end_ring_index"])
    np.testing.assert_array_equal(a["point_col_ind"], b["point_col_ind"])
    np.testing.assert_array_equal(bits(a["point_range"]), bits(b["point_range"]))
    np.testing.assert_array_equal(xyzi(a["cloud_deskewed"]).view(np.uint32), xyzi(b["cloud_deskewed"]).view(np.uint32))


# ----------------------------------------------------------------------------- a-0
def test_organize_bit_exact(pair, scene):
    o, g = pair
    _assert_info_equal(o.organize_scan(scene["scan"]), g.organize_scan(scene["scan"]))


def test_organize_edge_cases(pkg, oracle, hip):
    A = pkg._abi
    rng = np.random.default_rng(5)
    # tiny Horizon: columns past Horizon_SCAN are dropped; lines >= N_SCAN and out-of-range points are gated
    kw = dict(N_SCAN=4, Horizon_SCAN=100, max_raw_points=4096, max_map_points=1024)
    o = pkg.LidarHotpath(oracle, **kw); g = pkg.LidarHotpath(hip, **kw)
    pts = np.zeros(3001, A.LIVOX_DTYPE)
    pts["x"] = rng.uniform(-60, 60, 3001); pts["y"] = rng.uniform(-60, 60, 3001); pts["z"] = rng.uniform(-2, 5, 3001)
    pts["x"][::17] = 0.1; pts["y"][::17] = 0.1; pts["z"][::17] = 0.1          # below lidarMinRange
    pts["x"][5::23] = 500.0                                                   # beyond lidarMaxRange
    pts["line"] = rng.integers(0, 6, 3001)                                    # 4,5 are outside N_SCAN
    pts["reflectivity"] = rng.integers(0, 256, 3001)
    _assert_info_equal(o.organize_scan(pts), g.organize_scan(pts))
    for n in (0, 1, 2, 7):
        _assert_info_equal(o.organize_scan(pts[:n]), g.organize_scan(pts[:n]))
    # the final point of the message is dropped (imageProjection.cpp:249)
    one = pts[:2].copy(); one["x"] = 5; one["y"] = 0; one["z"] = 0; one["line"] = 0
    assert g.organize_scan(one)["n"] == 1
    o.close(); g.close()


# ----------------------------------------------------------------------------- f-1
def test_deskew_matches_oracle(pkg, oracle, hip):
    """IMU deskew inside organise: ranges / columns / ring bounds bit-exact; points bit-exact wherever the device's
    double-rounded sin/cos equal libm's (all but a handful of angles), within 2 ulp of the coordinate scale otherwise"""
    S = pkg.synth
    o = pkg.LidarHotpath(oracle, **small_params()); g = pkg.LidarHotpath(hip, **small_params())
    scan = S.make_scan(20001, S.loop_pose(0.7, 0.01, -0.02), 77)
    t0 = 1234.5
    t = np.arange(t0 - 0.003, t0 + 0.12, 1.0 / 200.0)
    rng = np.random.default_rng(3)
    w = np.cumsum(rng.normal(0, 0.3, (len(t), 3)), axis=0) * 0.05 + [0.3, -0.2, 0.9]          # wandering angular velocity
    rot = np.concatenate([[np.zeros(3)], np.cumsum(w[1:] * np.diff(t)[:, None], axis=0)])
    a = o.organize_scan_deskew(scan, t0, t, rot)
    b = g.organize_scan_deskew(scan, t0, t, rot)
    assert a["n"] == b["n"] > 15000
    for k in ("start_ring_index", "end_ring_index", "point_col_ind"):
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(bits(a["point_range"]), bits(b["point_range"]))
    pa, pb = xyzi(a["cloud_deskewed"]), xyzi(b["cloud_deskewed"])
    np.testing.assert_array_equal(pa[:, 3], pb[:, 3])
    assert np.abs(pa[:, :3] - pb[:, :3]).max() <= 4e-6 * np.abs(pa[:, :3]).max()
    assert (pa[:, :3].view(np.uint32) == pb[:, :3].view(np.uint32)).mean() > 0.98
    # and the whole path keeps working on the deskewed cloud (staged form)
    for h in (o, g):
        h.scan_set_deskew(t0, t, rot); h.scan_upload(scan); h.scan_organize(); h.scan_extract()
    (co, so), (cg, sg) = o.get_features(), g.get_features()
    assert len(co) == len(cg) and len(so) == len(sg)
    # plain organise afterwards is not deskewed
    np.testing.assert_array_equal(xyzi(o.organize_scan(scan)["cloud_deskewed"]).view(np.uint32), xyzi(g.organize_scan(scan)["cloud_deskewed"]).view(np.uint32))
    o.close(); g.close()


# ----------------------------------------------------------------------------- a-1..a-3
def test_smoothness_and_occlusion_bit_exact(pkg, pair, scene):
    A = pkg._abi
    o, g = pair
    for h in (o, g):
        h.scan_upload(scene["scan"]); h.scan_organize(); h.scan_extract()
    n = o.counts()["n"]
    co, cg = o.debug_get(A.DBG_CURVATURE, np.float32), g.debug_get(A.DBG_CURVATURE, np.float32)
    np.testing.assert_array_equal(bits(co[5:n - 5]), bits(cg[5:n - 5]))
    po, pg = o.debug_get(A.DBG_PICKED_OCCL, np.int32), g.debug_get(A.DBG_PICKED_OCCL, np.int32)
    np.testing.assert_array_equal(po[5:n - 5], pg[5:n - 5])


def test_feature_extraction_indices_bit_exact(pkg, pair, scene):
    A = pkg._abi
    o, g = pair
    for h in (o, g):
        h.scan_upload(scene["scan"]); h.scan_organize(); h.scan_extract()
    io, ig = o.debug_get(A.DBG_CORNER_INDEX, np.int32), g.debug_get(A.DBG_CORNER_INDEX, np.int32)
    assert len(io) > 50, "scene should produce corners"
    np.testing.assert_array_equal(io, ig)
    n = o.counts()["n"]
    lo, lg = o.debug_get(A.DBG_LABEL, np.int32), g.debug_get(A.DBG_LABEL, np.int32)
    np.testing.assert_array_equal(lo[5:n - 5], lg[5:n - 5])
    fo, fg = o.debug_get(A.DBG_PICKED_FINAL, np.int32), g.debug_get(A.DBG_PICKED_FINAL, np.int32)
    np.testing.assert_array_equal(fo[5:n - 6], fg[5:n - 6])
    (c_o, s_o), (c_g, s_g) = o.get_features(), g.get_features()
    np.testing.assert_array_equal(xyzi(c_o).view(np.uint32), xyzi(c_g).view(np.uint32))
    assert len(s_o) == len(s_g)
    np.testing.assert_allclose(xyzi(s_o), xyzi(s_g), rtol=0, atol=2e-5)


def test_second_scan_on_same_handle(pkg, pair, scene):
    """state that survives a scan must not change results vs the oracle"""
    A = pkg._abi
    o, g = pair
    S = pkg.synth
    scan2 = S.make_scan(20001, S.loop_pose(1.1, -0.01, 0.02), 999)
    for h in (o, g):
        for sc in (scene["scan"], scan2):
            h.scan_upload(sc); h.scan_organize(); h.scan_extract()
    np.testing.assert_array_equal(o.debug_get(A.DBG_CORNER_INDEX, np.int32), g.debug_get(A.DBG_CORNER_INDEX, np.int32))
    assert o.counts() == g.counts()


def test_extract_features_one_call_seam(pair, scene):
    o, g = pair
    info = o.organize_scan(scene["scan"])
    (c_o, s_o), (c_g, s_g) = o.extract_features(info), g.extract_features(info)
    np.testing.assert_array_equal(xyzi(c_o).view(np.uint32), xyzi(c_g).view(np.uint32))
    assert len(s_o) == len(s_g)
    np.testing.assert_allclose(xyzi(s_o), xyzi(s_g), rtol=0, atol=2e-5)


def test_sector_kernel_geometries(pkg, oracle, hip):
    """the pipelined (ring, sector) form, the sequential fallback for rings with a degenerate sector (fewer than 66
    points), empty rings, more rings than the default and the yaml's Horizon_SCAN: indices and labels exact"""
    S = pkg.synth
    A = pkg._abi
    base = S.make_scan(24001, S.loop_pose(0.9, 0.01, 0.02), 404)
    cases = []
    thin = base.copy()                                  # ring 3 keeps 40 points, ring 2 none
    idx3 = np.flatnonzero(thin["line"] == 3)
    thin["line"][idx3[40:]] = 9                         # an invalid line is dropped (imageProjection.cpp:586-588)
    thin["line"][thin["line"] == 2] = 9
    cases.append((dict(N_SCAN=4, Horizon_SCAN=8192), thin))
    six = base.copy(); six["line"] = (np.arange(len(six)) % 6).astype(np.uint8)
    cases.append((dict(N_SCAN=6, Horizon_SCAN=6000), six))          # yaml Horizon_SCAN, six rings
    tiny = base[:300].copy()                            # every ring degenerate
    cases.append((dict(N_SCAN=4, Horizon_SCAN=8192), tiny))
    for kw, scan in cases:
        P = dict(max_raw_points=40000, max_map_points=400000); P.update(kw)
        o = pkg.LidarHotpath(oracle, **P); g = pkg.LidarHotpath(hip, **P)
        for rep in range(2):                            # second scan on the same handles: not the "fresh node" case
            for h in (o, g):
                h.scan_upload(scan); h.scan_organize(); h.scan_extract()
            n = o.get_scan_info()["n"]
            np.testing.assert_array_equal(o.debug_get(A.DBG_CORNER_INDEX, np.int32), g.debug_get(A.DBG_CORNER_INDEX, np.int32))
            if n > 10:                                  # entries outside [5, n-5) are never reset by the reference (stale across scans) and never read
                np.testing.assert_array_equal(o.debug_get(A.DBG_LABEL, np.int32)[5:n - 5], g.debug_get(A.DBG_LABEL, np.int32)[5:n - 5])
                np.testing.assert_array_equal(o.debug_get(A.DBG_PICKED_FINAL, np.int32)[5:n - 5], g.debug_get(A.DBG_PICKED_FINAL, np.int32)[5:n - 5])
            (co, so), (cg, sg) = o.get_features(), g.get_features()
            np.testing.assert_array_equal(xyzi(co).view(np.uint32), xyzi(cg).view(np.uint32))
            assert len(so) == len(sg)
        o.close(); g.close()


# ----------------------------------------------------------------------------- a-4
def _voxel_case(pkg, o, g, pts, leaf):
    A = pkg._abi
    vo, vg = o.voxel_downsample(pts, leaf), g.voxel_downsample(pts, leaf)
    ko, kg = o.debug_get(A.DBG_VOXEL_KEYS, np.int32), g.debug_get(A.DBG_VOXEL_KEYS, np.int32)
    np.testing.assert_array_equal(ko, kg)
    np.testing.assert_array_equal(o.debug_get(A.DBG_VOXEL_CELLS, np.int32), g.debug_get(A.DBG_VOXEL_CELLS, np.int32))
    cnt = o.debug_get(A.DBG_VOXEL_COUNTS, np.int32)
    np.testing.assert_array_equal(cnt, g.debug_get(A.DBG_VOXEL_COUNTS, np.int32))
    assert len(vo) == len(vg)
    if len(vo) and len(cnt) == 0:                      # PCL's overflow rule fired: output = input, bit for bit
        np.testing.assert_array_equal(xyzi(vo).view(np.uint32), xyzi(vg).view(np.uint32))
        np.testing.assert_array_equal(xyzi(vg).view(np.uint32), np.asarray(pts, np.float32).view(np.uint32))
    elif len(vo):
        assert np.all(np.abs(xyzi(vo).astype(np.float64) - xyzi(vg)) <= centroid_tol(cnt, vo))
    return len(vo)


def test_voxel_downsample_keys_bit_exact(pkg, pair):
    o, g = pair
    rng = np.random.default_rng(1)
    pts = np.zeros((30000, 4), np.float32)
    pts[:, :3] = rng.uniform(-40, 40, (30000, 3)) * [1, 1, 0.1]
    pts[:, 3] = rng.uniform(0, 255, 30000)
    for leaf in (0.4, 0.2, 1.0, 0.05):
        assert _voxel_case(pkg, o, g, pts, leaf) > 100
    # clustered (many points per voxel), negative-only and positive-only coordinates
    c = np.zeros((5000, 4), np.float32); c[:, :3] = rng.normal(0, 0.3, (5000, 3)) + [-7.3, 2.2, -1.1]
    _voxel_case(pkg, o, g, c, 0.4)
    _voxel_case(pkg, o, g, np.abs(c), 0.2)
    _voxel_case(pkg, o, g, -np.abs(c), 0.2)


def test_voxel_million_point_segments(pkg, oracle, hip):
    """segments of a million points and more (many tiles per bin, multi-chunk bins, vb_merge): keys, cells, counts and
    centroids as the oracle, identical bits from the binned and the sorted path"""
    kw = dict(N_SCAN=4, Horizon_SCAN=1000, max_raw_points=4096, max_map_points=1400000)
    o = pkg.LidarHotpath(oracle, **kw)
    gb, gs = pkg.LidarHotpath(hip, voxel_mode=2, **kw), pkg.LidarHotpath(hip, voxel_mode=1, **kw)
    rng = np.random.default_rng(8)
    for n in ((1 << 20) - 1, 1 << 20, 1300007):
        pts = np.zeros((n, 4), np.float32)
        t = np.sort(rng.uniform(0, 1, n))                  # scan-line order with jumps, as a fused keyframe map
        pts[:, 0] = 60 * np.cos(40 * t) * rng.uniform(0.2, 1, n); pts[:, 1] = 60 * np.sin(40 * t) * rng.uniform(0.2, 1, n)
        pts[:, 2] = rng.uniform(-2, 6, n); pts[:, 3] = rng.uniform(0, 255, n)
        _voxel_case(pkg, o, gb, pts, 0.4)
        vb, vs = gb.voxel_downsample(pts, 0.4), gs.voxel_downsample(pts, 0.4)
        np.testing.assert_array_equal(xyzi(vb).view(np.uint32), xyzi(vs).view(np.uint32))
    o.close(); gb.close(); gs.close()


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["vox_auto", "vox_sorted", "vox_binned"])
def test_voxel_modes_ragged_sizes_and_sparse_grids(pkg, oracle, hip, mode):
    """ragged sizes around the wave / tile boundaries, compact grids (1024-voxel bins), sparse huge grids (wide bins
    swept per occupied sub-range) and the overflow rule, per realisation; auto switches after the first batch"""
    kw = dict(N_SCAN=4, Horizon_SCAN=1000, max_raw_points=4096, max_map_points=20000)
    o = pkg.LidarHotpath(oracle, **kw); g = pkg.LidarHotpath(hip, voxel_mode=mode, **kw)
    rng = np.random.default_rng(21)
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 20000):
        pts = np.zeros((n, 4), np.float32)
        pts[:, :3] = rng.uniform(-25, 25, (n, 3)) * [1, 1, 0.2]
        pts[:, 3] = rng.uniform(0, 255, n)
        for leaf in (0.4, 0.1, 3.0, 0.02):
            _voxel_case(pkg, o, g, pts, leaf)
    # scan-line order (runs of points in the same voxel, as in a keyframe cloud) and a constant intensity
    t = np.linspace(0, 40, 20000, dtype=np.float32)
    line = np.stack([t - 20, np.sin(t) * 5, 0.1 * t, np.full_like(t, 3.0)], axis=1).astype(np.float32)
    assert _voxel_case(pkg, o, g, line, 0.4) > 50
    far = np.array([[0, 0, 0, 1], [3000, 3000, 3000, 2], [1, 1, 1, 3]], np.float32)
    np.testing.assert_array_equal(xyzi(g.voxel_downsample(far, 0.01)), far)
    assert len(g.voxel_downsample(np.zeros((0, 4), np.float32), 0.4)) == 0
    o.close(); g.close()


def test_voxel_modes_give_identical_bits(pkg, hip):
    """integer sums commute: the sorted and the binned realisation return the same floats"""
    kw = dict(N_SCAN=4, Horizon_SCAN=1000, max_raw_points=4096, max_map_points=60000)
    a = pkg.LidarHotpath(hip, voxel_mode=1, **kw); b = pkg.LidarHotpath(hip, voxel_mode=2, **kw)
    rng = np.random.default_rng(5)
    pts = np.zeros((60000, 4), np.float32)
    pts[:, :3] = rng.normal(0, 6, (60000, 3)) * [1, 1, 0.2]
    pts[:, 3] = rng.uniform(-5, 300, 60000)
    for leaf in (0.4, 0.2, 0.03):
        ra, rb = xyzi(a.voxel_downsample(pts, leaf)), xyzi(b.voxel_downsample(pts, leaf))
        np.testing.assert_array_equal(ra.view(np.uint32), rb.view(np.uint32))
    a.close(); b.close()


def test_voxel_small_cloud_form_gives_the_general_path_bits(pkg, hip, monkeypatch):
    """round 3: a cloud of at most 1 024 points (the node's key-pose grid, mapOptimization.cpp:894-929) is filtered by ONE workgroup in one
    launch; same output bits, voxel idx and counts as the nine-launch general path (LVI_VOX_NO_TINY=1), incl. the overflow rule, one
    point, all points in one voxel, and key-pose-like input (a trajectory with a 2 m leaf)"""
    A = pkg._abi
    kw = dict(N_SCAN=4, Horizon_SCAN=1000, max_raw_points=4096, max_map_points=20000)
    rng = np.random.default_rng(33)
    cases = []
    for n in (1, 2, 5, 64, 65, 300, 777, 1024):
        pts = np.zeros((n, 4), np.float32)
        pts[:, :3] = rng.uniform(-25, 25, (n, 3)) * [1, 1, 0.2]; pts[:, 3] = rng.uniform(0, 255, n)
        for leaf in (0.4, 2.0, 0.02, 30.0):
            cases.append((pts, leaf))
    t = np.linspace(0, 60, 400, dtype=np.float32)
    cases.append((np.stack([t, np.sin(0.2 * t) * 8, 0.02 * t, np.arange(400, dtype=np.float32)], axis=1).astype(np.float32), 2.0))   # key poses, intensity = index
    cases.append((np.repeat(np.array([[1.5, -2.5, 0.25, 7.0]], np.float32), 1024, axis=0), 0.4))
    cases.append((np.array([[0, 0, 0, 1], [3000, 3000, 3000, 2], [1, 1, 1, 3]], np.float32), 0.01))                                   # overflow rule
    out = []
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("LVI_VOX_NO_TINY", env)
        else:
            monkeypatch.delenv("LVI_VOX_NO_TINY", raising=False)
        g = pkg.LidarHotpath(hip, **kw)
        rows = []
        for pts, leaf in cases:
            v = xyzi(g.voxel_downsample(pts, leaf)).view(np.uint32).copy()
            rows.append((v, g.debug_get(A.DBG_VOXEL_CELLS, np.int32).copy(), g.debug_get(A.DBG_VOXEL_COUNTS, np.int32).copy(), g.debug_get(A.DBG_VOXEL_KEYS, np.int32).copy()))
        out.append(rows)
        g.close()
    monkeypatch.delenv("LVI_VOX_NO_TINY", raising=False)
    for (a, b), (pts, leaf) in zip(zip(*out), cases):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y, err_msg=f"n={len(pts)} leaf={leaf}")


def test_voxel_downsample_edge_cases(pkg, pair):
    o, g = pair
    assert len(g.voxel_downsample(np.zeros((0, 4), np.float32), 0.4)) == 0
    one = np.array([[1.5, -2.5, 0.25, 7.0]], np.float32)
    np.testing.assert_array_equal(xyzi(g.voxel_downsample(one, 0.4)), one)
    same = np.repeat(one, 100, axis=0)
    r = xyzi(g.voxel_downsample(same, 0.4))
    assert r.shape == (1, 4) and np.allclose(r, one, atol=1e-5)
    # PCL overflow rule: dx*dy*dz > INT32_MAX -> output is the input, unchanged and in order
    far = np.array([[0, 0, 0, 1], [3000, 3000, 3000, 2], [1, 1, 1, 3], [-3000, 10, 10, 4]], np.float32)
    ro, rg = o.voxel_downsample(far, 0.01), g.voxel_downsample(far, 0.01)
    np.testing.assert_array_equal(xyzi(ro), far)
    np.testing.assert_array_equal(xyzi(rg), far)


# ----------------------------------------------------------------------------- a-5
def test_transform_cloud(pair, scene):
    o, g = pair
    pts = scene["map_surf"][:5000]
    pose = [0.02, -0.03, 1.2, 3.0, -4.0, 0.5]
    # a fixed-order f32 expression (a*x + b*y + c*z + d, mapOptimization.cpp:360-363) over the same 3x4 matrix: bit for bit.
    # (The matrix entries come from sin / cos: the HIP path rounds the double result, glibc's sinf / cosf are correctly rounded
    # for these angles; the soak of round 1 covers angles where they are not.)
    np.testing.assert_array_equal(xyzi(o.transform_cloud(pts, pose)).view(np.uint32), xyzi(g.transform_cloud(pts, pose)).view(np.uint32))


# ----------------------------------------------------------------------------- a-4(map) + a-6
def test_map_build_and_knn_exact(pkg, pair, scene):
    o, g = pair
    for h in (o, g):
        h.map_set(scene["map_corner"], scene["map_surf"])
    co, cg = o.counts(), g.counts()
    assert co["map_corner_ds"] == cg["map_corner_ds"] and co["map_surf_ds"] == cg["map_surf_ds"]
    (mco, mso), (mcg, msg) = o.get_map_ds(), g.get_map_ds()
    # centroid sum order differs (PCL: unspecified; here 32 lanes per map voxel): count * 2^-23 * max|coord|
    np.testing.assert_allclose(xyzi(mco), xyzi(mcg), rtol=0, atol=3e-4)
    np.testing.assert_allclose(xyzi(mso), xyzi(msg), rtol=0, atol=3e-4)
    # queries: map points jittered (dense neighbourhoods) + far-away points (rejected)
    rng = np.random.default_rng(3)
    for which, m in ((0, mcg), (1, msg)):
        # give the oracle exactly the GPU's DS map so that index parity is meaningful
        q = xyzi(m)[rng.integers(0, len(m), 4000)].copy()
        q[:, :3] += rng.normal(0, 0.15, (4000, 3)).astype(np.float32)
        q[-200:, :3] += 50.0
        io, do = o.debug_knn(which, q)
        ig, dg = g.debug_knn(which, q)
        accepted = io[:, 4] >= 0
        assert accepted.sum() > 500
        # maps can differ in the last bit of a centroid; distances then differ by rounding, indices must not
        mism = (io != ig).any(axis=1)
        assert mism.mean() < 2e-3, f"{mism.sum()} of {len(q)} queries differ"
        np.testing.assert_allclose(do[~mism], dg[~mism], rtol=1e-4, atol=1e-6)
    # ---- the identical-input leg: both libraries index the SAME DS map — the HIP path's, handed over as a raw
    # map (one point per voxel: its centroid is the point itself on both sides) — and then nothing is tolerated: indices and
    # squared distances bit for bit
    for h in (o, g):
        h.map_set(mcg, msg)
    (aco, aso), (acg, asg) = o.get_map_ds(), g.get_map_ds()
    np.testing.assert_array_equal(xyzi(aco).view(np.uint32), xyzi(acg).view(np.uint32))
    np.testing.assert_array_equal(xyzi(aso).view(np.uint32), xyzi(asg).view(np.uint32))
    # that holds because no coordinate lies in the near-zero band, where a one-point voxel is the model, not the point
    for raw, ds, leaf in ((mcg, acg, 0.2), (msg, asg, 0.4)):
        np.testing.assert_array_equal(xyzi(ds).view(np.uint32), centroid_ref.model_centroids(raw, leaf)["pts"].view(np.uint32))
    for which, m in ((0, acg), (1, asg)):
        q = xyzi(m)[rng.integers(0, len(m), 4000)].copy()
        q[:, :3] += rng.normal(0, 0.15, (4000, 3)).astype(np.float32)
        q[-200:, :3] += 50.0
        io, do = o.debug_knn(which, q)
        ig, dg = g.debug_knn(which, q)
        assert (io[:, 4] >= 0).sum() > 500
        # a genuine distance tie between two map points may be listed in either order by the kd-tree: compare as (distance, index) sets
        tie = (do[:, 1:] == do[:, :-1]).any(axis=1) & (io[:, 4] >= 0)
        np.testing.assert_array_equal(io[~tie], ig[~tie])
        np.testing.assert_array_equal(bits(do), bits(dg))
        np.testing.assert_array_equal(np.sort(io[tie], axis=1), np.sort(ig[tie], axis=1))


def test_knn_index_bit_exact_on_identical_map(pkg, oracle, hip):
    """one map point per voxel → oracle (f32 running sums) and HIP (exact mean) give identical centroids → KNN must match exactly"""
    rng = np.random.default_rng(11)
    P = small_params()
    o = pkg.LidarHotpath(oracle, **P); g = pkg.LidarHotpath(hip, **P)
    m = np.zeros((60000, 4), np.float32)
    m[:, :3] = (rng.integers(-200, 200, (60000, 3)) * 0.25 + 0.125) * [1, 1, 0.2]      # one point per 0.2-voxel at most twice
    m = np.unique(m, axis=0)
    _, first = np.unique(np.floor(m[:, :3] / np.float32(0.4)).astype(np.int64), axis=0, return_index=True)
    m = m[np.sort(first)]                                                               # at most one point per 0.4-voxel (and per 0.2-voxel)
    assert len(m) > 20000
    # a one-point voxel is the point itself only outside the near-zero band (bits finer than the 2^-k grid)
    assert np.abs(m[:, :3]).min() >= 2.0 ** (23 - min(centroid_ref.fx_k(0.2), centroid_ref.fx_k(0.4)))
    for h in (o, g):
        h.map_set(m, m)
    (mco, mso), (mcg, msg) = o.get_map_ds(), g.get_map_ds()
    np.testing.assert_array_equal(xyzi(mco), xyzi(mcg))
    np.testing.assert_array_equal(xyzi(mso), xyzi(msg))
    q = np.zeros((6000, 4), np.float32)
    q[:, :3] = rng.uniform(-50, 50, (6000, 3)) * [1, 1, 0.2] + rng.normal(0, 1e-3, (6000, 3))
    for which in (0, 1):
        io, do = o.debug_knn(which, q)
        ig, dg = g.debug_knn(which, q)
        ties = np.array([len(np.unique(r[np.isfinite(r)])) < np.isfinite(r).sum() for r in do])
        ok = ~ties
        np.testing.assert_array_equal(io[ok], ig[ok])
        np.testing.assert_array_equal(bits(do[ok]), bits(dg[ok]))
    o.close(); g.close()


# ----------------------------------------------------------------------------- f-4
def test_map_assemble_matches_oracle(pkg, oracle, hip, scene):
    """keyframes resident on the device, fused by index list: the raw fused clouds are bit-identical to the oracle's
    (same host-side libm matrix, same f32 expression), everything downstream as for lvi_map_set"""
    A = pkg._abi
    S = pkg.synth
    o = pkg.LidarHotpath(oracle, **small_params()); g = pkg.LidarHotpath(hip, **small_params())
    kfs = []
    for k in range(6):
        pose = S.loop_pose(0.25 + 0.04 * k, 0.01, -0.01).astype(np.float32)
        o.scan_upload(S.make_scan(20001, pose, 500 + k)); o.scan_organize(); o.scan_extract(); o.scan_downsample()
        c, s = o.get_scan_ds()
        kfs.append((c.copy(), s.copy(), pose))
    for h in (o, g):
        for c, s, pose in kfs:
            h.keyframe_add(c, s, pose)
        assert h.keyframe_count()[0] == 6
    order = [5, 2, 0, 3, 1, 4, 2]
    for h in (o, g):
        h.map_assemble(order)
    for what in (A.DBG_MAP_CORNER_RAW, A.DBG_MAP_SURF_RAW):
        np.testing.assert_array_equal(xyzi(o.debug_get(what, A.PT_DTYPE)).view(np.uint32), xyzi(g.debug_get(what, A.PT_DTYPE)).view(np.uint32))
    (mco, mso), (mcg, msg) = o.get_map_ds(), g.get_map_ds()
    assert len(mco) == len(mcg) and len(mso) == len(msg) > 2000
    np.testing.assert_allclose(xyzi(mso), xyzi(msg), rtol=0, atol=3e-4)
    # scan matching against the assembled map
    res = []
    for h in (o, g):
        h.scan_upload(scene["scan"]); h.scan_organize(); h.scan_extract(); h.scan_downsample()
        res.append(h.scan_match(scene["guess"]))
    assert res[0]["status"] == res[1]["status"] == 0
    dp = np.abs(res[0]["pose"] - res[1]["pose"])
    assert dp[:3].max() < 1e-4 and dp[3:].max() < 1e-4
    # the current scan becomes a keyframe without leaving the device
    for h, r in zip((o, g), res):
        assert h.keyframe_add_current(res[0]["pose"]) == 6
        h.map_assemble([6, 0])
    ro, rg = xyzi(o.debug_get(A.DBG_MAP_SURF_RAW, A.PT_DTYPE)), xyzi(g.debug_get(A.DBG_MAP_SURF_RAW, A.PT_DTYPE))
    assert ro.shape == rg.shape
    np.testing.assert_allclose(ro, rg, rtol=0, atol=3e-4)          # scan DS centroids differ by the documented tolerance
    o.close(); g.close()


# ----------------------------------------------------------------------------- a-7, a-8
def test_residuals_at_fixed_pose(pkg, pair, scene):
    o, g = pair
    for h in (o, g):
        h.map_set(scene["map_corner"], scene["map_surf"])
        h.scan_upload(scene["scan"]); h.scan_organize(); h.scan_extract(); h.scan_downsample()
    assert o.counts() == g.counts()
    for which in (0, 1):
        co, fo = o.debug_residuals(which, scene["guess"])
        cg, fg = g.debug_residuals(which, scene["guess"])
        assert fo.sum() > (20 if which == 0 else 1000)
        both = (fo == 1) & (fg == 1)
        assert (fo != fg).mean() < 5e-3, f"flag mismatch {(fo != fg).sum()} / {len(fo)}"
        d = np.abs(xyzi(co)[both] - xyzi(cg)[both])
        assert np.quantile(d, 0.999) < 2e-3 and np.median(d) < 1e-5, (np.quantile(d, 0.999), np.median(d))
    # ---- the identical-input leg: the same DS map and the same DS scan on both sides (the HIP path's, handed
    # over as raw clouds with one point per voxel).  Then the neighbours are the same and the selection flags must be EQUAL; the
    # coefficients differ only by the rounding of the two eigen / QR restatements
    (mcg, msg), (scg, ssg) = g.get_map_ds(), g.get_scan_ds()
    for h in (o, g):
        h.map_set(mcg, msg)
        h.scan_to_map(scg, ssg, scene["guess"])                   # uploads the clouds as features, second-stage DS, match
    assert o.counts()["corner_ds"] == g.counts()["corner_ds"] == len(scg) and o.counts()["surf_ds"] == g.counts()["surf_ds"] == len(ssg)
    for a, b in zip(o.get_scan_ds(), g.get_scan_ds()):
        np.testing.assert_array_equal(xyzi(a).view(np.uint32), xyzi(b).view(np.uint32))
    for which in (0, 1):
        co, fo = o.debug_residuals(which, scene["guess"])
        cg, fg = g.debug_residuals(which, scene["guess"])
        np.testing.assert_array_equal(fo, fg)
        both = fo == 1
        d = np.abs(xyzi(co)[both] - xyzi(cg)[both])
        assert d.max() < 2e-4 and np.median(d) < 1e-6, (d.max(), np.median(d))


# ----------------------------------------------------------------------------- a-9, a-10
def test_scan_to_map_pose_parity(pkg, pair, scene):
    A = pkg._abi
    o, g = pair
    for h in (o, g):
        h.map_set(scene["map_corner"], scene["map_surf"])
        h.scan_upload(scene["scan"]); h.scan_organize(); h.scan_extract(); h.scan_downsample()
    ro, rg = o.scan_match(scene["guess"]), g.scan_match(scene["guess"])
    assert ro["status"] == 0 and rg["status"] == 0
    assert ro["converged"] and rg["converged"]
    assert ro["degenerate"] == rg["degenerate"]
    assert ro["iters"] == rg["iters"]
    assert max(abs(a - b) for a, b in zip(ro["n_sel"], rg["n_sel"])) <= 3
    dp = np.abs(ro["pose"] - rg["pose"])
    assert dp[:3].max() < 1e-4 and dp[3:].max() < 1e-4, dp
    # and both land on the ground truth up to sensor noise
    assert np.abs(rg["pose"][3:] - scene["pose"][3:]).max() < 0.03
    assert np.abs(rg["pose"][:3] - scene["pose"][:3]).max() < 0.003
    jo, jg = o.debug_get(A.DBG_ICP_JTJ, np.float32), g.debug_get(A.DBG_ICP_JTJ, np.float32)
    np.testing.assert_allclose(jo[:27], jg[:27], rtol=2e-3, atol=1e-2)
    # ---- the identical-input leg: the HIP path's DS map and DS scan on both sides: selected counts equal in
    # every iteration, the same number of iterations, poses far inside the bar
    (mcg, msg), (scg, ssg) = g.get_map_ds(), g.get_scan_ds()
    for h in (o, g):
        h.map_set(mcg, msg)
    xo, xg = o.scan_to_map(scg, ssg, scene["guess"]), g.scan_to_map(scg, ssg, scene["guess"])
    assert xo["status"] == xg["status"] == 0 and xo["iters"] == xg["iters"] and xo["degenerate"] == xg["degenerate"]
    np.testing.assert_array_equal(np.array(xo["n_sel"]), np.array(xg["n_sel"]))
    assert np.abs(xo["pose"] - xg["pose"]).max() < 2e-5, np.abs(xo["pose"] - xg["pose"])
    # … and the 27 sums of EVERY recorded iteration (each one's solve is pinned to float64 in tests/test_gpu_step.py)
    jo, jg = o.debug_get(A.DBG_ICP_JTJ, np.float32).reshape(-1, 27), g.debug_get(A.DBG_ICP_JTJ, np.float32).reshape(-1, 27)
    assert jo.shape == jg.shape == (xo["iters"], 27)
    to, tg = o.debug_get(A.DBG_ICP_POSE_TRACE, np.float32).reshape(-1, 6), g.debug_get(A.DBG_ICP_POSE_TRACE, np.float32).reshape(-1, 6)
    for it in range(len(jo)):
        print(f"identical-input leg, iteration {it}: |d pose| {np.abs(to[it] - tg[it]).max():.2e}  "
              f"max |d sums| / (1e-2 + 2e-3 |sums|) = {(np.abs(jo[it] - jg[it]) / (1e-2 + 2e-3 * np.abs(jg[it]))).max():.3e}")
        np.testing.assert_allclose(jo[it], jg[it], rtol=2e-3, atol=1e-2, err_msg=f"iteration {it}")
    for h in (o, g):
        h.map_set(scene["map_corner"], scene["map_surf"])
    # IMU hint path (transformUpdate slerp) and the one-call seam: a hint 0.1 / -0.2 rad off the unhinted result moves roll and
    # pitch 1 % of the way (imuRPYWeight 0.01) on either library — a device that ignored the hint would miss by 1e-3 / 2e-3.
    # (tests/test_gpu_update.py pins the update itself to a closed form.)
    c, s = o.get_features()
    r1o, r1g = o.scan_to_map(c, s, scene["guess"]), g.scan_to_map(c, s, scene["guess"])
    assert r1o["status"] == r1g["status"] == 0
    r2 = []
    for h, r1 in ((o, r1o), (g, r1g)):
        imu = dict(imu_available=1, roll=float(r1["pose"][0]) + 0.1, pitch=float(r1["pose"][1]) - 0.2, yaw=0.0)
        r = h.scan_to_map(c, s, scene["guess"], imu)
        assert abs((r["pose"][0] - r1["pose"][0]) - 0.001) < 2e-5 and abs((r["pose"][1] - r1["pose"][1]) + 0.002) < 2e-5, (r["pose"], r1["pose"])
        np.testing.assert_array_equal(bits(r["pose"][2:]), bits(r1["pose"][2:]))
        r2.append(r)
    assert np.abs(r2[0]["pose"] - r2[1]["pose"]).max() < 1e-4


def test_scan_match_soft_outcomes(pkg, pair, scene):
    A = pkg._abi
    o, g = pair
    for h in (o, g):
        h.scan_upload(scene["scan"]); h.scan_organize(); h.scan_extract(); h.scan_downsample()
        assert h.scan_match(scene["guess"])["status"] == A.LVI_NO_MAP
    # a map far away from the scan: no correspondences -> LMOptimization never runs
    far_c = scene["map_corner"].copy(); far_s = scene["map_surf"].copy()
    far_c["x"] += 500; far_s["x"] += 500
    for h in (o, g):
        h.map_set(far_c, far_s)
        r = h.scan_match(scene["guess"])
        assert r["status"] == A.LVI_TOO_FEW_CORRESPONDENCES and r["iters"] == 20 and max(r["n_sel"]) < 50
        np.testing.assert_array_equal(bits(r["pose"]), bits(scene["guess"]))     # transformUpdate of the guess itself: no hint, tolerances of 1000
    # too few features
    few = scene["map_corner"][:5]
    for h in (o, g):
        r = h.scan_to_map(few, few, scene["guess"])
        assert r["status"] == A.LVI_TOO_FEW_FEATURES


def test_fixed_iteration_mode(pkg, oracle, hip, scene):
    """throughput runs disable the convergence break on CPU and GPU alike (SURVEY §8 d)"""
    P = small_params(icp_max_iters=10, icp_disable_break=1)
    o = pkg.LidarHotpath(oracle, **P); g = pkg.LidarHotpath(hip, **P)
    for h in (o, g):
        h.map_set(scene["map_corner"], scene["map_surf"])
        h.scan_upload(scene["scan"]); h.scan_organize(); h.scan_extract(); h.scan_downsample()
    ro, rg = o.scan_match(scene["guess"]), g.scan_match(scene["guess"])
    assert ro["iters"] == 10 and rg["iters"] == 10
    assert np.abs(ro["pose"] - rg["pose"]).max() < 1e-4
    o.close(); g.close()


def test_map_on_main_stream_gives_identical_results(pkg, hip, scene):
    """lvi_lidar_params.map_on_main_stream only moves the map build between streams: same bits out"""
    res = []
    for mode in (0, 1):
        g = pkg.LidarHotpath(hip, map_on_main_stream=mode, **small_params())
        g.map_upload(scene["map_corner"], scene["map_surf"])
        for rep in range(2):                               # the second round re-voxelises while the first index is still in use
            g.map_build()
            g.scan_upload(scene["scan"]); g.scan_organize(); g.scan_extract(); g.scan_downsample()
            r = g.scan_match(scene["guess"])
        res.append((r["pose"].copy(), np.array(r["n_sel"]), xyzi(g.get_map_ds()[1]).copy()))
        g.close()
    np.testing.assert_array_equal(bits(res[0][0]), bits(res[1][0]))
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(res[0][2].view(np.uint32), res[1][2].view(np.uint32))


def test_queue_depth_two_gives_the_same_records(pkg, hip, scene):
    """lvi_lidar_mark / lvi_lidar_wait_mark: scans enqueued back to back without a host sync (depth 2, either map
    stream) write the same pose records as scan-by-scan with lvi_lidar_sync"""
    import ctypes as C
    rt = C.CDLL("libamdhip64.so.7")                          # the runtime liblvi_hip.so is linked against (torch brings its own copy)
    rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipFree.argtypes = [C.c_void_p]
    H2D, D2H = 1, 2

    def dev_alloc(nbytes):
        p = C.c_void_p()
        assert rt.hipMalloc(C.byref(p), nbytes) == 0
        return p

    S = pkg.synth
    scans = [S.make_scan(12000, S.loop_pose(0.3 + 0.5 * k, 0.0, 0.0), 400 + k) for k in range(4)]
    guesses = [S.perturbed_guess(S.loop_pose(0.3 + 0.5 * k, 0.0, 0.0), 50 + k) for k in range(4)]
    d_scans = []
    for sc in scans:
        buf = np.ascontiguousarray(sc)
        p = dev_alloc(buf.nbytes)
        assert rt.hipMemcpy(p, buf.ctypes.data, buf.nbytes, H2D) == 0
        d_scans.append(p)
    d_rec = dev_alloc(len(scans) * 32)
    out = []
    for depth, stream_mode in ((1, 0), (2, 0), (2, 1)):
        g = pkg.LidarHotpath(hip, map_on_main_stream=stream_mode, **small_params())
        g.map_upload(scene["map_corner"], scene["map_surf"])
        zero = np.zeros((len(scans), 8), np.float32)
        assert rt.hipMemcpy(d_rec, zero.ctypes.data, zero.nbytes, H2D) == 0
        for i in range(len(scans)):
            if depth == 1:
                g.sync()
            else:
                g.wait_mark(i % depth)
            g.map_build()
            g.scan_upload_device(d_scans[i].value, len(scans[i]))
            g.scan_organize(); g.scan_extract(); g.scan_downsample()
            g.scan_match_async(guesses[i], d_rec.value + 32 * i)
            g.mark(i % depth)
        for s in range(depth):
            g.wait_mark(s)
        g.wait_mark(7)                                     # never marked: returns at once
        rec = np.zeros((len(scans), 8), np.float32)        # no lvi_lidar_sync before this read: the marks alone cover it
        assert rt.hipMemcpy(rec.ctypes.data, d_rec, rec.nbytes, D2H) == 0
        out.append(rec)
        with pytest.raises(Exception):
            g.mark(8)
        g.sync(); g.close()
    for p in d_scans + [d_rec]:
        rt.hipFree(p)
    assert (out[0][:, 6].view(np.int32) == 0).all()
    np.testing.assert_array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
    np.testing.assert_array_equal(out[0].view(np.uint32), out[2].view(np.uint32))


def test_parity_sweep_over_scans_and_settings(pkg, oracle, hip, scene):
    """the whole path on a dozen different scans / poses / thresholds: selected indices exact, poses within the bar"""
    S = pkg.synth
    A = pkg._abi
    rng = np.random.default_rng(99)
    worst = 0.0
    for case in range(12):
        kw = small_params()
        if case % 3 == 1:
            kw.update(edgeThreshold=0.5, surfThreshold=0.2)
        if case % 3 == 2:
            kw.update(odometrySurfLeafSize=0.3, mappingSurfLeafSize=0.5, mappingCornerLeafSize=0.25)
        o = pkg.LidarHotpath(oracle, **kw); g = pkg.LidarHotpath(hip, voxel_mode=case % 3, **kw)
        pose = S.loop_pose(rng.uniform(0, 6.28), rng.normal(0, 0.02), rng.normal(0, 0.02))
        scan = S.make_scan(int(rng.integers(9000, 24000)), pose, 7000 + case)
        guess = S.perturbed_guess(pose, 100 + case)
        for h in (o, g):
            h.map_set(scene["map_corner"], scene["map_surf"])
            h.scan_upload(scan); h.scan_organize(); h.scan_extract(); h.scan_downsample()
        np.testing.assert_array_equal(o.debug_get(A.DBG_CORNER_INDEX, np.int32), g.debug_get(A.DBG_CORNER_INDEX, np.int32))
        np.testing.assert_array_equal(o.debug_get(A.DBG_LABEL, np.int32), g.debug_get(A.DBG_LABEL, np.int32))
        co, cg = o.counts(), g.counts()
        # second-stage grids (scan DS of the ring centroids) see inputs that differ by the centroid tolerance: a centroid
        # within ~1e-6 m of a voxel face may change voxel, so that count is compared loosely; first-stage counts are exact
        assert abs(co.pop("surf_ds") - cg.pop("surf_ds")) <= 3, (case, co, cg)
        assert co == cg, (case, co, cg)
        ro, rg = o.scan_match(guess), g.scan_match(guess)
        assert ro["status"] == rg["status"] and ro["iters"] == rg["iters"], (case, ro, rg)
        if ro["status"] == 0:
            dp = np.abs(ro["pose"] - rg["pose"])
            assert dp[:3].max() < 1e-4 and dp[3:].max() < 1e-4, (case, dp)
            worst = max(worst, float(dp.max()))
        o.close(); g.close()
    assert worst < 1e-4


# ----------------------------------------------------------------------------- full size
def test_full_size_scan_properties(pkg, oracle, hip):
    """BASELINE config sizes: 100k-pt scan; size-independent properties + oracle on the scan stages"""
    A = pkg._abi
    S = pkg.synth
    P = dict(N_SCAN=4, Horizon_SCAN=32768, max_raw_points=131072, max_map_points=1 << 20)
    o = pkg.LidarHotpath(oracle, **P); g = pkg.LidarHotpath(hip, **P)
    scan = S.make_scan(100001, S.loop_pose(2.2, 0.01, 0.0), 12345)
    for h in (o, g):
        h.scan_upload(scan); h.scan_organize(); h.scan_extract(); h.scan_downsample()
    assert o.counts() == g.counts()
    np.testing.assert_array_equal(o.debug_get(A.DBG_CORNER_INDEX, np.int32), g.debug_get(A.DBG_CORNER_INDEX, np.int32))
    info = g.get_scan_info()
    assert info["n"] == 100000
    # columns are a dense per-ring counter; ranges are inside the gate
    for r in range(4):
        b = info["start_ring_index"][r] - 4
        e = info["end_ring_index"][r] + 6
        np.testing.assert_array_equal(info["point_col_ind"][b:e], np.arange(e - b))
    assert info["point_range"].min() >= 1.0 and info["point_range"].max() <= 100.0
    # voxel idempotence: downsampling an already downsampled cloud with the same leaf keeps the count
    cds, sds = g.get_scan_ds()
    again = g.voxel_downsample(sds, 0.4)
    assert abs(len(again) - len(sds)) <= 0.02 * len(sds)
    o.close(); g.close()


# ----------------------------------------------------------------------------- one-call replay (hipGraph)
def test_replay_enqueue_matches_staged_path(pkg, oracle, hip, scene):
    """lvi_scan_replay_enqueue (captured launch sequence, map rebuilt per scan) == the staged calls == the oracle"""
    import ctypes as C
    P = small_params(icp_max_iters=10, icp_disable_break=1)
    o = pkg.LidarHotpath(oracle, **P); g = pkg.LidarHotpath(hip, **P); g2 = pkg.LidarHotpath(hip, **P)
    S = pkg.synth
    scans = [scene["scan"], S.make_scan(20001, S.loop_pose(1.3, 0.0, 0.01), 321)]
    guesses = [scene["guess"], S.perturbed_guess(S.loop_pose(1.3, 0.0, 0.01), 9)]
    for h in (o, g, g2):
        h.map_upload(scene["map_corner"], scene["map_surf"])
    # the replay entry point wants the scan in device memory: borrow the handle g's own raw buffer through a
    # second handle's upload → not available from Python, so stage it via hipMalloc from the HIP runtime
    hiprt = C.CDLL("libamdhip64.so.7")
    for rep in range(3):                         # first call captures, later calls replay the graph
        for sc, gs in zip(scans, guesses):
            o.map_build(); o.scan_upload(sc); o.scan_organize(); o.scan_extract(); o.scan_downsample()
            ro = o.scan_match(gs)
            g.map_build(); g.scan_upload(sc); g.scan_organize(); g.scan_extract(); g.scan_downsample()
            rg = g.scan_match(gs)
            dptr = C.c_void_p()
            assert hiprt.hipMalloc(C.byref(dptr), C.c_size_t(sc.nbytes)) == 0
            assert hiprt.hipMemcpy(dptr, sc.ctypes.data_as(C.c_void_p), C.c_size_t(sc.nbytes), 1) == 0
            g2.scan_replay_enqueue(dptr.value, len(sc), gs, 0, rebuild_map=True)
            rr = g2.get_pose_record()
            hiprt.hipFree(dptr)
            assert rr["status"] == 0 and rr["iters"] == 10
            np.testing.assert_array_equal(rr["pose"], rg["pose"])            # same kernels, same order → bitwise
            assert np.abs(rr["pose"] - ro["pose"]).max() < 1e-4
            assert g2.counts() == g.counts()
    o.close(); g.close(); g2.close()


# ----------------------------------------------------------------------------- BASELINE config 3 at full size
@pytest.fixture(scope="module")
def bench_map(pkg, hip):
    """the raw local map of bench.py (BASELINE config 3: ~4.87 M points from 250 synthetic keyframes), from the same
    generator and seed: the HIP handle extracts the keyframe features (bench.py ray-casts with torch on the GPU, here numpy)"""
    S = pkg.synth
    P = dict(N_SCAN=4, Horizon_SCAN=32768, max_raw_points=131072, max_map_points=1 << 16)
    g = pkg.LidarHotpath(hip, **P)
    mc, ms = S.make_map(g, 250, 30001, seed=4711, target_surf=5_000_000)
    g.close()
    assert len(ms) > 4_000_000
    return mc, ms


FULL = dict(N_SCAN=4, Horizon_SCAN=32768, max_raw_points=131072, max_map_points=5_000_000 + 65536)


def test_full_size_map_voxel_grids(pkg, oracle, hip, bench_map):
    """the 4.87 M-point surf map through VoxelGrid(0.4) and the corner map through VoxelGrid(0.2): voxel idx per point, set of
    occupied cells, points per cell and output order bit for bit; centroids inside count * 2^-23 * max|coord|"""
    mc, ms = bench_map
    o = pkg.LidarHotpath(oracle, **FULL); g = pkg.LidarHotpath(hip, **FULL)
    assert _voxel_case(pkg, o, g, xyzi(ms), 0.4) > 50_000
    assert _voxel_case(pkg, o, g, xyzi(mc), 0.2) > 1_000
    o.close(); g.close()


@pytest.mark.parametrize("fixed", [True, False], ids=["ten_fixed_iterations", "reference_break"])
def test_full_size_scan_to_map(pkg, oracle, hip, bench_map, fixed):
    """BASELINE config 3: 100 001-point scans against the bench's raw map, (a) 10 iterations with the break disabled (what
    bench.py times) and (b) reference semantics (<= 20, break): DS counts exact, status / iteration count equal, pose within
    1e-4 m / 1e-4 rad, selected counts within a few knife-edge features of ~15 000 (a feature whose weight s or plane
    distance sits on its threshold follows the last bit of the pose; with identical inputs the test asserts that every
    count moves by at most 0.1 % and that the poses agree)."""
    S = pkg.synth
    mc, ms = bench_map
    kw = dict(FULL)
    if fixed:
        kw.update(icp_max_iters=10, icp_disable_break=1)
    o = pkg.LidarHotpath(oracle, **kw); g = pkg.LidarHotpath(hip, **kw)
    for h in (o, g):
        h.map_upload(mc, ms); h.map_build()
    co, cg = o.counts(), g.counts()
    assert co["map_corner_ds"] == cg["map_corner_ds"] and co["map_surf_ds"] == cg["map_surf_ds"] > 50_000
    worst = _full_size_scans(S, o, g, fixed, exact_surf_ds=False)
    print(f"full-size scan-to-map ({'10 fixed' if fixed else 'reference'} iterations): worst |pose_hip - pose_oracle| = {worst:.2e}")
    # the same scans with the oracle's VoxelGrids on the HIP centroid contract: the second-stage grid then sees
    # identical ring-DS centroids on both sides, so its count is exact
    d = oracle.dll
    d.lvo_set_centroid_mode.argtypes = [ctypes.c_int]
    d.lvo_set_centroid_mode(1)
    try:
        worst1 = _full_size_scans(S, o, g, fixed, exact_surf_ds=True)
    finally:
        d.lvo_set_centroid_mode(0)
    print(f"  oracle centroids on the HIP contract: surf_ds exact, worst |pose_hip - pose_oracle| = {worst1:.2e}")
    o.close(); g.close()


def _full_size_scans(S, o, g, fixed, exact_surf_ds):
    """bench.py's scan pool of rank 0 (same poses, seeds, guesses) through both handles: DS counts, status, iterations,
    selected counts and pose; returns the worst pose difference"""
    worst = 0.0
    for sid in range(3):
        pose = S.loop_pose(0.37 + 0.71 * sid, 0.01 * np.sin(sid), -0.02 * np.cos(sid))
        scan = S.make_scan(100001, pose, 12345 + sid)
        guess = S.perturbed_guess(pose, sid)
        for h in (o, g):
            h.map_build()                                        # the reference re-voxelises and re-indexes per scan
            h.scan_upload(scan); h.scan_organize(); h.scan_extract(); h.scan_downsample()
        co, cg = o.counts(), g.counts()
        if exact_surf_ds:
            assert co["surf_ds"] == cg["surf_ds"], (co, cg)
        else:
            assert abs(co.pop("surf_ds") - cg.pop("surf_ds")) <= 3, (co, cg)     # second-stage grid: see test_parity_sweep_…
        assert co == cg, (co, cg)
        ro, rg = o.scan_match(guess), g.scan_match(guess)
        assert ro["status"] == rg["status"] == 0
        assert ro["iters"] == rg["iters"], (ro["iters"], rg["iters"])
        if fixed:
            assert rg["iters"] == 10
        assert ro["degenerate"] == rg["degenerate"]
        gap = max(abs(a - b) for a, b in zip(ro["n_sel"], rg["n_sel"]))
        assert min(rg["n_sel"]) > 5000 and gap <= max(3, int(1e-3 * max(ro["n_sel"]))), (ro["n_sel"], rg["n_sel"])
        dp = np.abs(ro["pose"] - rg["pose"])
        assert dp[:3].max() < 1e-4 and dp[3:].max() < 1e-4, (sid, dp)
        worst = max(worst, float(dp.max()))
        assert np.abs(rg["pose"][3:] - pose[3:]).max() < 0.05 and np.abs(rg["pose"][:3] - pose[:3]).max() < 0.01
    return worst


# ----------------------------------------------------------------------------- sector pipeline robustness
def test_sector_redo_path_gives_identical_bits(pkg, hip, scene):
    """sector_handover_wait_us < 0: no pipelined sector workgroup ever waits for its predecessor, every one walks the ring
    from sector 0 itself — the self-rescue of a workgroup whose producer is not resident.  Same bits as the pipeline."""
    A = pkg._abi
    out = []
    for wait in (0, -1):
        g = pkg.LidarHotpath(hip, sector_handover_wait_us=wait, **small_params())
        rows = []
        for rep in range(2):
            g.scan_upload(scene["scan"]); g.scan_organize(); g.scan_extract()
            n = g.counts()["n"]
            rows.append((g.debug_get(A.DBG_CORNER_INDEX, np.int32), g.debug_get(A.DBG_LABEL, np.int32)[5:n - 5],
                         g.debug_get(A.DBG_PICKED_FINAL, np.int32)[5:n - 5], xyzi(g.get_features()[1]).view(np.uint32).copy()))
        out.append(rows)
        g.close()
    for ra, rb in zip(out[0], out[1]):
        for x, y in zip(ra, rb):
            np.testing.assert_array_equal(x, y)


def test_many_handles_in_flight(pkg, hip, scene):
    """16 handles x 24 pipelined sector workgroups (each owning a CU's LDS) enqueued back to back on 16 streams: more waiting
    consumers than the chip has CUs is survivable (bounded wait, then redo) and every handle returns the same record"""
    H = 16
    hs = [pkg.LidarHotpath(hip, icp_max_iters=4, icp_disable_break=1, **small_params(max_map_points=120000)) for _ in range(H)]
    mc, ms = scene["map_corner"], scene["map_surf"][:100000]
    for h in hs:
        h.map_upload(mc, ms); h.map_build()
    for h in hs:
        h.sync()
    for rep in range(3):
        for h in hs:                                       # nothing synchronises between the handles
            h.scan_upload(scene["scan"]); h.scan_organize(); h.scan_extract(); h.scan_downsample()
            h.scan_match_async(scene["guess"], 0)
    recs = [h.get_pose_record() for h in hs]
    for r in recs:
        assert r["status"] == 0 and r["iters"] == 4
        np.testing.assert_array_equal(bits(r["pose"]), bits(recs[0]["pose"]))
    for h in hs:
        h.close()


def test_oversize_sectors_take_the_global_memory_walk(pkg, oracle, hip, scene):
    """N_SCAN = 1 with 60 000 points: sectors of 10 000 points exceed the LDS-resident sector kernel (FEAT_SEG_CAP = 8 192); such
    rings go through feat_sector_big_kernel (same two walks over global memory).  Indices, labels, picked flags and the whole
    path as the oracle; a mixed scan (one oversize ring next to ordinary ones) too"""
    A, S = pkg._abi, pkg.synth
    for n_scan, lines in ((1, lambda sc: 0), (3, lambda sc: np.where(np.arange(len(sc)) % 10 < 8, 0, 1 + np.arange(len(sc)) % 2))):
        P = dict(N_SCAN=n_scan, Horizon_SCAN=65536, max_raw_points=70000, max_map_points=400000)
        o = pkg.LidarHotpath(oracle, **P); g = pkg.LidarHotpath(hip, **P)
        for h in (o, g):
            h.map_set(scene["map_corner"], scene["map_surf"])
        for rep in range(2):                                        # fresh handle, then reused
            pose = S.loop_pose(0.37 + 0.3 * rep, 0.01, -0.02)
            scan = S.make_scan(60001, pose, 5 + rep)
            scan["line"] = lines(scan)
            for h in (o, g):
                h.scan_upload(scan); h.scan_organize(); h.scan_extract(); h.scan_downsample()
            n = o.counts()["n"]
            np.testing.assert_array_equal(o.debug_get(A.DBG_CORNER_INDEX, np.int32), g.debug_get(A.DBG_CORNER_INDEX, np.int32))
            np.testing.assert_array_equal(o.debug_get(A.DBG_LABEL, np.int32)[5:n - 5], g.debug_get(A.DBG_LABEL, np.int32)[5:n - 5])
            np.testing.assert_array_equal(o.debug_get(A.DBG_PICKED_FINAL, np.int32)[5:n - 6], g.debug_get(A.DBG_PICKED_FINAL, np.int32)[5:n - 6])
            co, cg = o.counts(), g.counts()
            assert abs(co.pop("surf_ds") - cg.pop("surf_ds")) <= 3 and co == cg, (co, cg)
            ro, rg = o.scan_match(S.perturbed_guess(pose, rep)), g.scan_match(S.perturbed_guess(pose, rep))
            assert ro["status"] == rg["status"] == 0 and ro["iters"] == rg["iters"]
            assert np.abs(ro["pose"] - rg["pose"]).max() < 1e-4
        o.close(); g.close()


# ----------------------------------------------------------------------------- batched launches
def _dev_buffers(arrays):
    """copy host arrays to device memory through the HIP runtime liblvi_hip.so links (no torch needed)"""
    import ctypes as C
    rt = C.CDLL("libamdhip64.so.7")
    rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipFree.argtypes = [C.c_void_p]
    ptrs = []
    for a in arrays:
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert rt.hipMalloc(C.byref(p), max(a.nbytes, 16)) == 0
        assert rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        ptrs.append(p)
    return rt, ptrs


@pytest.mark.parametrize("rebuild", [True, False], ids=["map_rebuilt_per_scan", "frozen_map"])
def test_batched_launches_are_bit_identical(pkg, hip, scene, rebuild):
    """lvi_scan_batch_*: S scans of different sizes side by side in one launch sequence (slot in blockIdx.z) give, slot by
    slot, the bits of the single-scan entry points: pose records, counts, corner indices, labels, DS clouds, DS map"""
    A = pkg._abi
    S = pkg.synth
    NB = 4
    P = small_params(icp_max_iters=10, icp_disable_break=1)
    sizes = [20001, 12000, 17003, 9001]
    poses = [S.loop_pose(0.37 + 0.6 * k, 0.01 * k, -0.01) for k in range(NB)]
    scans = [S.make_scan(sizes[k], poses[k], 900 + k) for k in range(NB)]
    guesses = np.stack([S.perturbed_guess(poses[k], 20 + k) for k in range(NB)])
    # ---- reference: one scan at a time on a plain handle
    g = pkg.LidarHotpath(hip, **P)
    g.map_upload(scene["map_corner"], scene["map_surf"]); g.map_build()
    ref = []
    for k in range(NB):
        if rebuild:
            g.map_build()
        g.scan_upload(scans[k]); g.scan_organize(); g.scan_extract(); g.scan_downsample()
        g.scan_match_async(guesses[k], 0)
        rec = g.get_pose_record()
        ref.append(dict(rec=rec, counts=g.counts(), ci=g.debug_get(A.DBG_CORNER_INDEX, np.int32), lab=g.debug_get(A.DBG_LABEL, np.int32),
                        ds=[xyzi(c).view(np.uint32).copy() for c in g.get_scan_ds()], mapds=[xyzi(c).view(np.uint32).copy() for c in g.get_map_ds()]))
    g.close()
    # ---- the same four scans as one batch (device-resident scans bound in place, then host scans through staging)
    b = pkg.LidarHotpath(hip, batch_scans=NB, **P)
    b.map_upload(scene["map_corner"], scene["map_surf"]); b.map_build()
    rt, ptrs = _dev_buffers(scans)
    for form in ("bind", "upload"):
        for rep in range(2):
            if form == "bind":
                b.batch_bind_device([p.value for p in ptrs], sizes)
            else:
                b.batch_upload(scans)
            b.batch_run(guesses, 0, rebuild_map=rebuild)
            recs = b.batch_get_records(NB)
            for k in range(NB):
                np.testing.assert_array_equal(recs[k, :6].view(np.uint32), ref[k]["rec"]["pose"].view(np.uint32))
                assert int(recs[k, 6:7].view(np.int32)[0]) == 0 and int(recs[k, 7:8].view(np.int32)[0]) == 10
                b.batch_select(k)
                assert b.counts() == ref[k]["counts"], (k, b.counts(), ref[k]["counts"])
                np.testing.assert_array_equal(b.debug_get(A.DBG_CORNER_INDEX, np.int32), ref[k]["ci"])
                n = ref[k]["counts"]["n"]
                np.testing.assert_array_equal(b.debug_get(A.DBG_LABEL, np.int32)[5:n - 5], ref[k]["lab"][5:n - 5])
                for x, y in zip(b.get_scan_ds(), ref[k]["ds"]):
                    np.testing.assert_array_equal(xyzi(x).view(np.uint32), y)
                for x, y in zip(b.get_map_ds(), ref[k]["mapds"]):
                    np.testing.assert_array_equal(xyzi(x).view(np.uint32), y)
            b.batch_select(0)
    # a partial batch (fewer scans than slots) and a batch of one
    b.batch_upload(scans[1:3]); b.batch_run(guesses[1:3], 0, rebuild_map=rebuild)
    recs = b.batch_get_records(2)
    for j, k in enumerate((1, 2)):
        np.testing.assert_array_equal(recs[j, :6].view(np.uint32), ref[k]["rec"]["pose"].view(np.uint32))
    with pytest.raises(pkg.LviError):
        b.batch_upload(scans + scans[:1])                 # more scans than batch_scans
    for p in ptrs:
        rt.hipFree(p)
    b.close()


def test_knn_radius_bound_gives_identical_bits(pkg, hip, scene, monkeypatch):
    """from the second GN iteration on the 5-NN search is bounded by the previous neighbours' distances under the new pose
    (exact: five map points lie inside that ball), and skipped altogether when the lower bound the feature's last search left
    on the distance to every OTHER map point proves that the five are still the five nearest (several slack radii, incl. 0).
    Same records, selected counts and JtJ bits as searching the unit ball in every iteration"""
    A = pkg._abi
    S = pkg.synth
    out = []
    # … and the same whether a wavefront searches its LDS tile of the index or global memory (LVI_KNN_TILES=1), with 64 or 256
    # features per workgroup (LVI_ICP_WIDE_FROM), with 2, 4 or 8 lanes per feature
    modes = (dict(LVI_KNN_NO_BOUND="1"), dict(LVI_KNN_NO_SKIP="1"), dict(), dict(LVI_KNN_SLACK="0"), dict(LVI_KNN_SLACK="0.2"), dict(LVI_ICP_G1="2"),
             dict(LVI_KNN_TILES="1"), dict(LVI_KNN_TILES="1", LVI_KNN_NO_BOUND="1"), dict(LVI_ICP_WIDE_FROM="1"), dict(LVI_ICP_WIDE_FROM="99", LVI_ICP_G0="8"),
             dict(LVI_ICP_G0="2", LVI_ICP_G1="8"),
             # … and whatever the launch grid: sized for the capacity, or for far fewer features than the scan has (every workgroup then
             # walks on through several blocks of features), with 64 and with 256 features per block
             dict(LVI_GN_GRID="cap"), dict(LVI_GN_GRID_FEATURES="300"), dict(LVI_GN_GRID_FEATURES="1100", LVI_ICP_WIDE_FROM="1"))
    ALL = ("LVI_KNN_NO_BOUND", "LVI_KNN_NO_SKIP", "LVI_KNN_SLACK", "LVI_ICP_G1", "LVI_ICP_G0", "LVI_KNN_TILES", "LVI_ICP_WIDE_FROM", "LVI_GN_GRID",
           "LVI_GN_GRID_FEATURES")
    for env in modes:
        for k in ALL:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        rows, searches = [], []
        for kw in (dict(), dict(icp_max_iters=10, icp_disable_break=1)):
            g = pkg.LidarHotpath(hip, **small_params(**kw))
            g.map_set(scene["map_corner"], scene["map_surf"])
            for k in range(3):
                pose = S.loop_pose(0.37 + 0.8 * k, 0.01, -0.02)
                g.scan_upload(S.make_scan(20001 - 3000 * k, pose, 60 + k)); g.scan_organize(); g.scan_extract(); g.scan_downsample()
                r = g.scan_match(S.perturbed_guess(pose, 5 + k))
                rows.append((bits(r["pose"]), np.array(r["n_sel"]), r["iters"], bits(g.debug_get(A.DBG_ICP_JTJ, np.float32))))
                cyc = g.debug_get(A.DBG_ICP_CYCLES, np.int64)
                c = g.counts()
                searches.append((int(cyc[15]), (c["corner_ds"] + c["surf_ds"]) * r["iters"]))
            g.close()
        out.append((rows, searches))
    for k in ALL:
        monkeypatch.delenv(k, raising=False)
    for rows, _ in out[1:]:
        for ra, rb in zip(out[0][0], rows):
            for x, y in zip(ra, rb):
                np.testing.assert_array_equal(x, y)
    # without the skip every feature searches in every iteration; with it most of the later iterations do not
    for (n, full) in out[0][1] + out[1][1]:
        assert n == full
    frac = sum(n for n, _ in out[2][1]) / sum(f for _, f in out[2][1])
    assert frac < 0.7, frac


def test_map_share_reads_the_owner_map_in_place(pkg, hip, scene):
    """lvi_map_share: a second handle (also a batch handle) matches against the raw map another handle holds — same bits as
    with its own upload; its own upload afterwards ends the sharing and leaves the owner's map alone"""
    S = pkg.synth
    pose = S.loop_pose(0.37, 0.01, -0.02)
    scan = S.make_scan(20001, pose, 60)
    guess = S.perturbed_guess(pose, 5)

    def match(g):
        g.scan_upload(scan); g.scan_organize(); g.scan_extract(); g.scan_downsample()
        r = g.scan_match(guess)
        return bits(r["pose"]), np.array(r["n_sel"]), r["iters"], g.counts()["map_surf_ds"]

    owner = pkg.LidarHotpath(hip, **small_params())
    owner.map_set(scene["map_corner"], scene["map_surf"])
    ref = match(owner)
    b = pkg.LidarHotpath(hip, **small_params())
    with pytest.raises(Exception):
        b.map_share(b)
    b.map_share(owner); b.map_build()
    got = match(b)
    for x, y in zip(ref, got):
        np.testing.assert_array_equal(x, y)
    # a batch handle sharing the same map
    bb = pkg.LidarHotpath(hip, **small_params(batch_scans=2))
    bb.map_share(owner)
    bb.batch_upload([scan, scan])
    bb.batch_run(np.stack([guess, guess]), rebuild_map=True)
    recs = bb.batch_get_records(2)
    for z in range(2):
        np.testing.assert_array_equal(bits(recs[z, :6]), ref[0])
    bb.close()
    # a launch sequence captured against b's OWN map (same sizes) must not survive the switch to the shared one
    c = pkg.LidarHotpath(hip, **small_params(icp_max_iters=6, icp_disable_break=1))
    shifted_c, shifted_s = scene["map_corner"].copy(), scene["map_surf"].copy()
    shifted_c["x"] += 0.5; shifted_s["x"] += 0.5
    c.map_set(shifted_c, shifted_s)
    import torch
    d_scan = torch.from_numpy(scan.view(np.uint8).copy()).to("cuda")
    d_rec = torch.zeros(8, dtype=torch.float32, device="cuda")
    c.scan_replay_enqueue(d_scan.data_ptr(), len(scan), guess, d_rec.data_ptr(), True); c.sync()
    own = d_rec.cpu().numpy().copy()
    o6 = pkg.LidarHotpath(hip, **small_params(icp_max_iters=6, icp_disable_break=1))
    o6.map_set(scene["map_corner"], scene["map_surf"])
    o6.scan_replay_enqueue(d_scan.data_ptr(), len(scan), guess, d_rec.data_ptr(), True); o6.sync()
    want = d_rec.cpu().numpy().copy()
    assert not np.array_equal(bits(own[:6]), bits(want[:6]))
    c.map_share(o6)
    c.scan_replay_enqueue(d_scan.data_ptr(), len(scan), guess, d_rec.data_ptr(), True); c.sync()
    np.testing.assert_array_equal(bits(d_rec.cpu().numpy()[:6]), bits(want[:6]))
    c.close(); o6.close()
    # the owner cannot change its map while it is shared
    with pytest.raises(pkg.LviError):
        owner.map_upload(scene["map_corner"], scene["map_surf"])
    # b uploads a different map of its own: the owner still matches against the first one
    half_c, half_s = scene["map_corner"][: len(scene["map_corner"]) // 2], scene["map_surf"][: len(scene["map_surf"]) // 2]
    b.map_set(half_c, half_s)
    assert b.counts()["map_surf_ds"] < ref[3]
    owner.map_build()
    again = match(owner)
    for x, y in zip(ref, again):
        np.testing.assert_array_equal(x, y)
    owner.map_upload(scene["map_corner"], scene["map_surf"])          # nobody shares it any more
    b.close(); owner.close()


# ----------------------------------------------------------------------------- decisions on a threshold (hand-built cases)
def test_corner_eigenvalue_ratio_gate(pkg, oracle, hip):
    """cornerOptimization accepts a line only if the largest eigenvalue of the 5-neighbour covariance exceeds 3x the second
    (mapOptimization.cpp:1052).  Clusters built so that the ratio is KNOWN (five points on a cross: variance a^2 2/5 along x,
    b^2 2/5 along y → ratio (a/b)^2) sweep the gate from 2 to 4.5; away from the threshold the decision is the analytic one in
    both libraries, and the two libraries agree everywhere (Jacobi in f32 on both sides; cv::eigen itself is not available:
    parity unpinned).
    These clusters are AXIS-ALIGNED: the covariance is diagonal, `eig3_sym` leaves before its first rotation, and what is tested
    at the gate is the ordering of three diagonal entries.  The crosses in rotated planes (full covariances, 5 / 60 / 250 m from
    the origin, both exact eigenvalue ties) are tests/test_gpu_fit.py::test_flags_on_hand_built_scenes, against float64"""
    P = dict(N_SCAN=4, Horizon_SCAN=2048, max_raw_points=8192, max_map_points=65536, mappingCornerLeafSize=0.05)
    o = pkg.LidarHotpath(oracle, **P); g = pkg.LidarHotpath(hip, **P)
    ratios = np.concatenate([np.linspace(2.0, 2.9, 10), [2.97, 2.99, 2.999, 3.001, 3.01, 3.03], np.linspace(3.1, 4.5, 10)])
    b = 0.12
    clusters, queries, expect = [], [], []
    for i, r in enumerate(ratios):
        a = b * np.sqrt(r)
        c = np.array([6.0 * (i % 6) - 15.0, 6.0 * (i // 6) - 12.0, 1.0])
        clusters += [c, c + [a, 0, 0], c - [a, 0, 0], c + [0, b, 0], c - [0, b, 0]]
        queries.append(c + [0.02, 0.03, 0.05])
        expect.append(r > 3.0)
    m = np.zeros((len(clusters), 4), np.float32); m[:, :3] = np.array(clusters)
    q = np.zeros((len(queries), 4), np.float32); q[:, :3] = np.array(queries)
    pad = np.zeros((200, 4), np.float32); pad[:, :3] = np.random.default_rng(0).uniform(200, 300, (200, 3))      # far-away filler
    flags = []
    for h in (o, g):
        h.map_set(np.concatenate([m, pad]), np.concatenate([m, pad]))
        assert h.counts()["map_corner_ds"] == len(m) + len(pad)          # 5 cm leaf: nothing merged
        r = h.scan_to_map(q, np.concatenate([q, pad[:150]]), np.zeros(6, np.float32))      # corner queries = the cluster centres, identity pose
        _, fl = h.debug_residuals(0, np.zeros(6, np.float32))
        flags.append(fl[:len(q)].astype(bool))
    np.testing.assert_array_equal(flags[0], flags[1])
    clear = np.abs(ratios - 3.0) > 0.02
    np.testing.assert_array_equal(flags[1][clear], np.array(expect)[clear])
    o.close(); g.close()


# ----------------------------------------------------------------------------- round 3: map plan per rebuild, advisor regressions
def _map_ds_bits(g):
    return [xyzi(c).view(np.uint32).copy() for c in g.get_map_ds()]


def test_map_plan_per_rebuild_matches_cached_plan(pkg, hip, scene):
    """lvi_lidar_params.map_plan_cache: 0 (default) takes the bounding box and the per-bin counts inside EVERY re-voxelisation
    of the raw map (one pass, the counts under the previous run's grid geometry, re-taken when the geometry moved); 1 takes them
    once per upload.  Same DS map bits either way, for an unchanged map, a map that moved by half a metre (same size, other
    grid), a smaller map, and back; batch slots included."""
    mc, ms = scene["map_corner"], scene["map_surf"]
    sh_c, sh_s = mc.copy(), ms.copy()
    sh_c["x"] += 0.5; sh_s["x"] += 0.5; sh_c["z"] -= 0.7; sh_s["z"] -= 0.7
    maps = [(mc, ms), (mc, ms), (sh_c, sh_s), (mc[: len(mc) // 2], ms[: len(ms) // 3]), (mc, ms)]
    per, cached = pkg.LidarHotpath(hip, **small_params(voxel_mode=2)), pkg.LidarHotpath(hip, **small_params(voxel_mode=2, map_plan_cache=1))
    auto = pkg.LidarHotpath(hip, **small_params())                 # AUTO: first build sorted, then binned with the per-run plan
    for step, (c, s) in enumerate(maps):
        fresh = pkg.LidarHotpath(hip, **small_params(voxel_mode=1))
        fresh.map_set(c, s)
        want = _map_ds_bits(fresh)
        fresh.close()
        for g in (per, cached, auto):
            if step != 1:
                g.map_upload(c, s)
            g.map_build()                                           # step 1: a second build of the unchanged map (plan_ok path)
            for x, y in zip(_map_ds_bits(g), want):
                np.testing.assert_array_equal(x, y)
    per.close(); cached.close(); auto.close()
    # batch slots: every slot takes its own plan
    b = pkg.LidarHotpath(hip, **small_params(batch_scans=3, voxel_mode=2))
    ref = pkg.LidarHotpath(hip, **small_params(voxel_mode=1))
    for (c, s) in (maps[0], maps[2]):
        ref.map_set(c, s); want = _map_ds_bits(ref)
        b.map_upload(c, s); b.map_build(); b.map_build()
        for z in range(3):
            b.batch_select(z)
            for x, y in zip(_map_ds_bits(b), want):
                np.testing.assert_array_equal(x, y)
        b.batch_select(0)
    b.close(); ref.close()


@pytest.mark.parametrize("cache", [0, 1], ids=["plan_per_rebuild", "plan_cached"])
def test_replay_graph_does_not_survive_a_map_upload(pkg, hip, scene, cache):
    """advisor, round 2: a captured launch sequence (lvi_scan_replay_enqueue) froze whether the map plan passes are part of it;
    a re-upload of a DIFFERENT map of the same size must not replay it: the bits of a fresh handle"""
    import torch
    S = pkg.synth
    P = small_params(icp_max_iters=6, icp_disable_break=1, map_plan_cache=cache)
    pose = S.loop_pose(0.37, 0.01, -0.02)
    scan = S.make_scan(20001, pose, 61)
    guess = S.perturbed_guess(pose, 6)
    d_scan = torch.from_numpy(scan.view(np.uint8).copy()).to("cuda")
    d_rec = torch.zeros(8, dtype=torch.float32, device="cuda")
    mc, ms = scene["map_corner"], scene["map_surf"]
    sh_c, sh_s = mc.copy(), ms.copy()
    sh_c["y"] += 0.9; sh_s["y"] += 0.9
    d_c = torch.from_numpy(xyzi(sh_c).copy()).to("cuda"); d_s = torch.from_numpy(xyzi(sh_s).copy()).to("cuda")

    def run(h):
        h.scan_replay_enqueue(d_scan.data_ptr(), len(scan), guess, d_rec.data_ptr(), True); h.sync()
        return bits(d_rec.cpu().numpy()[:6]).copy(), _map_ds_bits(h)

    g = pkg.LidarHotpath(hip, **P)
    g.map_set(mc, ms)                                               # eager build: with cache = 1 the plan is cached now
    run(g); run(g)                                                  # captured without the plan passes (cache = 1), replayed once
    g.map_upload_device(d_c.data_ptr(), len(sh_c), d_s.data_ptr(), len(sh_s))
    got = run(g)
    f = pkg.LidarHotpath(hip, **P)
    f.map_upload(sh_c, sh_s)
    want = run(f)
    np.testing.assert_array_equal(got[0], want[0])
    for x, y in zip(got[1], want[1]):
        np.testing.assert_array_equal(x, y)
    g.close(); f.close()


def test_bound_scan_buffer_is_dropped_by_a_single_scan_upload(pkg, hip, scene):
    """advisor, round 2: lvi_scan_batch_bind_device leaves the slot reading the caller's buffer; a later single-scan upload on
    that slot must process the NEW scan"""
    S = pkg.synth
    a = S.make_scan(15001, S.loop_pose(0.4, 0.0, 0.0), 70)
    b = S.make_scan(12001, S.loop_pose(1.1, 0.01, 0.0), 71)
    rt, ptrs = _dev_buffers([a])
    h = pkg.LidarHotpath(hip, **small_params(batch_scans=2))
    h.batch_bind_device([ptrs[0].value], [len(a)])
    h.scan_upload(b)                                                # slot 0, the single-scan entry point
    h.scan_organize()
    got = h.get_scan_info()
    p = pkg.LidarHotpath(hip, **small_params())
    p.scan_upload(b); p.scan_organize()
    _assert_info_equal(got, p.get_scan_info())
    rt.hipFree(ptrs[0])
    h.close(); p.close()


def test_map_owner_destroyed_before_its_sharers(pkg, hip, scene):
    """advisor, round 2: destroying the owner of a shared raw map sends the sharers back to their own (empty) memory instead of
    leaving them with dangling pointers; a handle that is shared cannot itself share another one's map"""
    owner = pkg.LidarHotpath(hip, **small_params())
    owner.map_set(scene["map_corner"], scene["map_surf"])
    s1 = pkg.LidarHotpath(hip, **small_params()); s2 = pkg.LidarHotpath(hip, **small_params(batch_scans=2))
    s1.map_share(owner); s1.map_build(); s2.map_share(owner); s2.map_build()
    other = pkg.LidarHotpath(hip, **small_params())
    other.map_set(scene["map_corner"], scene["map_surf"])
    with pytest.raises(pkg.LviError):
        owner.map_share(other)                                      # owner is shared: it cannot become a sharer
    with pytest.raises(pkg.LviError):
        owner.map_update(np.zeros(0, np.int32))                     # … nor drop its raw map
    owner.close()                                                   # the sharers are detached here
    with pytest.raises(pkg.LviError):
        s1.map_build()                                              # no raw map any more: a clean error, not a fault
    s1.map_set(scene["map_corner"], scene["map_surf"])              # and the handle works on with a map of its own
    assert s1.counts()["map_surf_ds"] == other.counts()["map_surf_ds"]
    s2.map_share(other); s2.map_build()
    s1.close(); s2.close(); other.close()
