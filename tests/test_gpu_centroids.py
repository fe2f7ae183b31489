"""GPU tier: every HIP VoxelGrid realisation against the exact centroid contract (centroid_ref.py).

Bit for bit against model_centroids and within the stated bound of exact_centroids, in every voxel: lvi_voxel_downsample
in voxel_mode 0 / 1 / 2 and in its small-cloud form, the scan's DS clouds, the map rebuild and the incremental map over
30+ keyframe add / remove steps."""
import numpy as np
import pytest

import centroid_ref as R
from helpers import make_small_scene, small_params, xyzi

pytestmark = pytest.mark.gpu

F32 = np.float32
LEAVES = (0.4, 0.2, 0.1, 0.25, 0.02, 5.0)


class _Tally:
    """per test: voxels checked, voxels where the model is not the correctly rounded true mean, and the worst
    |model - exact| as a fraction of the stated bound; reported and checked by the test that made it"""

    def __init__(self, name):
        self.name, self.n, self.off, self.worst = name, 0, 0, 0.0

    def done(self, at_least):
        print(f"centroids {self.name}: {self.n} voxels bit-exact to the model, {self.off} with model != exact, "
              f"worst |model - exact| = {self.worst:.3f} of the bound")
        assert self.n >= at_least, (self.name, self.n)
        assert self.worst <= 1.0


def _check(pkg, g, pts, leaf, tag, tally, ki=None, got=None):
    """g's output for `pts` (or `got`) is the model bit for bit and the model is within the bound of the exact mean"""
    m = R.model_centroids(pts, leaf, ki)
    if got is None:
        got = g.voxel_downsample(pts, leaf)
        np.testing.assert_array_equal(g.debug_get(pkg._abi.DBG_VOXEL_COUNTS, np.int32), m["counts"], err_msg=tag)
    got = xyzi(got)
    assert len(got) == len(m["pts"]), tag
    bad = np.nonzero(np.any(got.view(np.uint32) != m["pts"].view(np.uint32), axis=1))[0]
    assert len(bad) == 0, f"{tag}: {len(bad)} of {len(got)} voxels differ from the model, first cell {m['cells'][bad[0]]} count " \
                          f"{m['counts'][bad[0]]}: got {got[bad[0]]} model {m['pts'][bad[0]]}"
    e = R.exact_centroids(pts, leaf)
    ok = R.within_bound(m["pts"], e, leaf, m["k"], m["ki"])
    assert ok.all(), f"{tag}: model outside the bound of the exact mean in {np.count_nonzero(~ok.all(axis=1))} voxels"
    diff = np.abs(m["pts"].astype(np.float64) - e)
    tally.n += len(got)
    tally.off += int(np.count_nonzero(np.any(m["pts"] != e, axis=1)))
    tally.worst = max(tally.worst, float((diff / (R.model_bound(leaf, m["k"], m["ki"]) + R.half_ulp(m["pts"]) + R.half_ulp(e))).max(initial=0)))
    return m


def _in_cell(rng, cell, n, leaf, lo=0.02, hi=0.98):
    """n f32 points whose PCL key is `cell`"""
    p = ((np.asarray(cell) + rng.uniform(lo, hi, (n, 3))) * leaf).astype(F32)
    assert (R.pcl_cells(p, leaf) == np.asarray(cell)).all()
    return p


def _midpoint_voxel(rng, leaf, cell, n, up, axis=0):
    """n points whose exact mean along `axis` lies 2^-k / (2 n) above or below an f32 rounding midpoint (exactly on it for
    even n): values of the f32 binade whose ulp is the 2^-k grid, in cell -1 (cancellation against cell * leaf) or 0"""
    k = R.fx_k(leaf)
    base = 2.0 ** (23 - k) * (1 + rng.integers(1, 1 << 20) * 2.0 ** -23)
    sgn = -1.0 if cell[axis] < 0 else 1.0
    a, b = F32(sgn * base), F32(sgn * (base + 2.0 ** -k))
    assert b - a == F32(sgn * 2.0 ** -k)
    p = _in_cell(rng, cell, n, leaf)
    nb = (n + (1 if up else -1)) // 2 if n % 2 else n // 2
    p[:, axis] = a
    p[:nb, axis] = b
    assert (R.pcl_cells(p, leaf) == np.asarray(cell)).all()
    return p


def _three_roundings(cell, leaf, S, n, k):
    """negative control: the finalisation as it was, int -> binary64, divide, add cell * leaf, convert to f32 (three to four
    roundings).  Used only to pick test voxels that tell it apart from the contract."""
    return F32(float(cell) * float(F32(leaf)) + np.ldexp(float(S) / float(n), -k))


def _discriminating_voxel(rng, leaf, cell, n, axis=0):
    """a midpoint voxel (as _midpoint_voxel) of n points whose exact mean the old three-rounding finalisation rounds the wrong
    way: searched over the base value and the side of the midpoint, then asserted"""
    k = R.fx_k(leaf)
    ml, _ = R.leaf_parts(leaf)
    C = cell[axis] * (ml << 12)
    for _ in range(400):
        up = bool(rng.integers(0, 2))
        p = _midpoint_voxel(rng, leaf, cell, n, up, axis)
        S = int(R.q_xyz(p[:, axis], np.full(n, cell[axis]), leaf, k).sum())
        if _three_roundings(cell[axis], leaf, S, n, k) != R.f32_of(C * n + S, n << k):
            return p
    raise AssertionError("no discriminating voxel found")


def _cloud(rng, leaf, big=False):
    parts = []
    cells = [(-1, -1, -1), (0, 0, 0), (-1, 0, -1), (0, -1, 0), (-3, 2, -5), (5, -4, 1), (-1, -1, 0), (2, 0, -1), (-2, -2, -2), (1, 1, 1)]
    for cell, n in zip(cells, (1, 2, 3, 7, 63, 64, 65, 1 << 10, 1 << 16, 5)):
        parts.append(_in_cell(rng, cell, n, leaf))
    # on and one ulp either side of the cell faces -2 .. 3 of every axis
    for ax in range(3):
        for c in range(-2, 4):
            f = F32(c * leaf)
            for v in (np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))):
                p = _in_cell(rng, (1, -2, 2), 3, leaf)
                p[:, ax] = v
                parts.append(p)
    # the near-zero band, on every axis, alone and among other points of cells -1 and 0
    for ax in range(3):
        for v in (1e-9, -1e-9, 3e-5, -3e-5, 1e-6, -1e-6, 2.0 ** -140, -(2.0 ** -140)):
            p = _in_cell(rng, (3, 3, 3), 1, leaf)
            p[:, ax] = v
            parts.append(p)
            q = _in_cell(rng, (-1 if v < 0 else 0, 4, 4), 5, leaf)
            q[0, ax] = v
            parts.append(q)
    # constructed means next to an f32 rounding midpoint
    for i, n in enumerate((3, 65, 1025, 1 << 16 | 1, 64)):
        for up in (False, True):
            parts.append(_midpoint_voxel(rng, leaf, (-1, 6 + i, 6 + up), n, up))
            parts.append(_midpoint_voxel(rng, leaf, (6 + i, 6 + up, -1), n, up, axis=2))
        parts.append(_midpoint_voxel(rng, leaf, (0, 6 + i, 8), n, True))
    # ... of which the old finalisation (three roundings) gets these wrong: cell -1, where cell * leaf cancels the offset
    parts.append(_discriminating_voxel(rng, leaf, (-1, 20, 20), 1 << 18 | 1))
    parts.append(_discriminating_voxel(rng, leaf, (20, 21, -1), 1 << 18 | 1, axis=2))
    if big:
        for up in (False, True):
            parts.append(_midpoint_voxel(rng, leaf, (-1, 12, 6 + up), 1 << 20 | 1, up))
        # 2^22 points at the largest offset of their voxel (the int64 headroom of the sums) and a 2^20-point random voxel
        top = np.nextafter(F32(8 * leaf), F32(-np.inf))
        p = np.full((1 << 22, 3), top, F32)
        p[::3] = np.nextafter(top, F32(-np.inf))
        assert (R.pcl_cells(p[:2], leaf) == 7).all()
        parts.append(p)
        parts.append(_in_cell(rng, (-4, 3, -4), 1 << 20, leaf, 0.001, 0.999))
    xyz = np.concatenate(parts)
    pts = np.zeros((len(xyz), 4), F32)
    pts[:, :3] = xyz
    pts[:, 3] = rng.uniform(-3, 255.99, len(xyz))
    pts[::7, 3] = 0
    pts[1::7, 3] = -rng.uniform(0, 2.0 ** -5, len(pts[1::7]))
    pts[2::7, 3] = rng.uniform(0, 2.0 ** -5, len(pts[2::7]))
    pts[3::7, 3] = F32(255.99)
    perm = rng.permutation(len(pts))
    return pts[perm]


def _far_cloud(rng, leaf):
    """coordinates out to +-2000 m on x, narrow on y and z so that PCL's overflow rule stays quiet"""
    n = 4000
    p = np.zeros((n, 4), F32)
    p[:, 0] = rng.uniform(-2000, 2000, n)
    p[:200, 0] = np.repeat(rng.uniform(-2000, 2000, 20), 10)
    span = 2.0 ** 31 / (4000.0 / leaf + 1)
    w = max(min(np.sqrt(span) * leaf * 0.5, 50.0), leaf)
    p[:, 1] = rng.uniform(-w, w, n)
    p[:, 2] = rng.uniform(-w, 0, n)
    p[:, 3] = rng.uniform(0, 255.99, n)
    assert not R.pcl_overflow(p[:, :3], leaf)
    return p


KW = dict(N_SCAN=4, Horizon_SCAN=1000, max_raw_points=4096, max_map_points=1 << 23)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["vox_auto", "vox_sorted", "vox_binned"])
def test_voxel_downsample_is_the_model(pkg, hip, mode):
    g = pkg.LidarHotpath(hip, voxel_mode=mode, **KW)
    rng = np.random.default_rng(100 + mode)
    t = _Tally(f"lvi_voxel_downsample voxel_mode {mode}")
    for leaf in LEAVES:
        _check(pkg, g, _cloud(rng, leaf), leaf, f"downsample leaf {leaf} mode {mode}", t)
        _check(pkg, g, _far_cloud(rng, leaf), leaf, f"downsample far leaf {leaf} mode {mode}", t)
    # one intensity of 1e5 coarsens the segment's intensity grid to 2^-20
    p = _cloud(rng, 0.4)
    p[5, 3] = 1e5
    assert _check(pkg, g, p, 0.4, f"downsample int1e5 mode {mode}", t)["ki"] == 20
    g.close()
    t.done(20_000)


def test_voxel_downsample_large_voxels(pkg, hip):
    """2^22 points in one voxel at its largest offset, 2^20 points in another, midpoint voxels of 2^20 + 1 points"""
    rng = np.random.default_rng(7)
    pts = _cloud(rng, 0.4, big=True)
    assert len(pts) > (1 << 22) + (1 << 21)
    kw = dict(KW, max_map_points=1 << 24)
    t = _Tally("large voxels, voxel_mode 0 / 1 / 2")
    for mode in (0, 1, 2):
        g = pkg.LidarHotpath(hip, voxel_mode=mode, **kw)
        m = _check(pkg, g, pts, 0.4, f"large mode {mode}", t)
        assert m["counts"].max() >= 1 << 22
        g.close()
    t.done(200)


def test_voxel_downsample_small_cloud_form(pkg, hip):
    """clouds of at most 1 024 points (one-workgroup form)"""
    g = pkg.LidarHotpath(hip, **KW)
    rng = np.random.default_rng(9)
    t = _Tally("lvi_voxel_downsample small-cloud form")
    for leaf in LEAVES:
        for n in (1, 3, 200, 1024):
            p = _cloud(rng, leaf)[:n]
            _check(pkg, g, p, leaf, f"small leaf {leaf} n {n}", t)
        mid = np.zeros((1023, 4), F32)
        mid[:, :3] = _midpoint_voxel(rng, leaf, (-1, 2, 2), 1023, True)
        mid[:, 3] = rng.uniform(0, 255.99, 1023)
        _check(pkg, g, mid, leaf, f"small midpoint leaf {leaf}", t)
    g.close()
    t.done(150)


def test_scan_and_map_ds_are_the_model(pkg, oracle, hip):
    """downsampleCurrentScan (get_scan_ds of get_features) and the map rebuild (get_map_ds of the raw map), small scene"""
    sc = make_small_scene(pkg, oracle)
    lc, ls = 0.2, 0.4                        # mappingCornerLeafSize, mappingSurfLeafSize
    tm, ts = _Tally("map rebuild (get_map_ds), voxel_mode 0 / 1 / 2"), _Tally("scan DS (get_scan_ds), voxel_mode 0 / 1 / 2")
    for mode in (0, 1, 2):
        g = pkg.LidarHotpath(hip, voxel_mode=mode, **small_params())
        g.map_set(sc["map_corner"], sc["map_surf"]); g.map_build()
        mc, ms = g.get_map_ds()
        _check(pkg, g, sc["map_corner"], lc, f"map_ds corner mode {mode}", tm, got=mc)
        _check(pkg, g, sc["map_surf"], ls, f"map_ds surf mode {mode}", tm, got=ms)
        g.scan_upload(sc["scan"]); g.scan_organize(); g.scan_extract(); g.scan_downsample()
        fc, fs = g.get_features()
        dc, ds = g.get_scan_ds()
        _check(pkg, g, fc, lc, f"scan_ds corner mode {mode}", ts, got=dc)
        _check(pkg, g, fs, ls, f"scan_ds surf mode {mode}", ts, got=ds)
        g.close()
    tm.done(150_000)
    ts.done(30_000)


def test_incremental_map_is_the_model_of_the_active_set(pkg, oracle, hip):
    """map_update over 34 keyframe add / remove steps: the DS maps equal the model of the current active set (ki = 29), so
    the subtraction of leaving keyframes is exact; a keyframe with intensities >= 256 takes the full path (segment scale)"""
    S = pkg.synth
    A = pkg._abi
    o = pkg.LidarHotpath(oracle, **small_params())
    kfs = []
    for k in range(12):
        pose = S.loop_pose(0.2 + 0.11 * k, 0.01 * np.sin(k), -0.01 * np.cos(k)).astype(np.float32)
        o.scan_upload(S.make_scan(16001, pose, 900 + k)); o.scan_organize(); o.scan_extract(); o.scan_downsample()
        c, s = o.get_scan_ds()
        kfs.append((c.copy(), s.copy(), pose))
    o.close()
    kw = small_params(max_keyframes=64, max_keyframe_points=600000)
    a = pkg.LidarHotpath(hip, **kw)          # incremental
    b = pkg.LidarHotpath(hip, **kw)          # full assembly: the raw active set
    for h in (a, b):
        for c, s, pose in kfs:
            h.keyframe_add(c, s, pose)
    hot = kfs[3][1].copy()
    xyzi(hot)[::5, 3] = 300.0
    for h in (a, b):
        assert h.keyframe_add(kfs[3][0], hot, kfs[3][2]) == 12
    rng = np.random.default_rng(21)
    cur = [0, 1, 2]
    steps = 0
    t = _Tally("incremental map (map_update), 34 steps")
    for step in range(34):
        if step == 20:
            keys = cur + [12]                                               # intensities >= 256: the documented fallback
        else:
            cur = sorted(set(cur) - set(rng.choice(cur, min(len(cur), rng.integers(0, 3)), replace=False).tolist())
                         | set(rng.integers(0, 12, rng.integers(1, 4)).tolist()))
            keys = cur
        a.map_update(keys); b.map_assemble(keys)
        raw = (b.debug_get(A.DBG_MAP_CORNER_RAW, A.PT_DTYPE), b.debug_get(A.DBG_MAP_SURF_RAW, A.PT_DTYPE))
        ki = None if 12 in keys else 29
        for got, r, leaf, w in zip(a.get_map_ds(), raw, (0.2, 0.4), ("corner", "surf")):
            _check(pkg, a, np.ascontiguousarray(xyzi(r)), leaf, f"map_update {w} step {step} keys {keys}", t, ki=ki, got=got)
        steps += 1
    assert steps >= 30
    a.close(); b.close()
    t.done(1_000_000)


def test_depth_window_is_the_model(pkg, oracle, hip):
    """the depth window's second VoxelGrid (lidar_callback, DepthRegister.get_cloud / debug_voxel): with the oracle's
    VoxelGrids on the HIP contract (lvo_set_centroid_mode(1)) the reference window holds the HIP path's fused cloud bit for
    bit, and the HIP window is the model of that fused cloud"""
    import ctypes
    import depth_ref as D
    d = oracle.dll
    d.lvo_set_centroid_mode.argtypes = [ctypes.c_int]
    reg = pkg.DepthRegister(hip, max_clouds=12, max_cloud_points=30000, max_features=150, lidar_skip=0)
    t = _Tally("depth window (DepthRegister.get_cloud), 16 callbacks")
    d.lvo_set_centroid_mode(1)
    try:
        W = D.Window(pkg, oracle, lidar_skip=0, window_s=5.0)
        rng = np.random.default_rng(31)
        for k in range(16):
            n = 20000
            cloud = np.stack([9.0 + rng.normal(0, 0.3, n), rng.uniform(-8, 8, n), rng.uniform(-6, 6, n), rng.uniform(0, 100, n)], 1)
            cloud = cloud.astype(F32)
            cloud[:200, 1:3] = rng.uniform(-1e-4, 1e-4, (200, 2))                   # points in the near-zero band
            pose = (0.3 * k * 0.25, 0.05 * k * 0.25, 0.0, 0.0, 0.01 * k, 0.02 * k)
            assert reg.lidar_callback(cloud, pose, 100.0 + 0.5 * k) and W.lidar_callback(cloud, pose, 100.0 + 0.5 * k)
            fused = np.concatenate(W.clouds)
            got = reg.get_cloud()
            cells, counts = reg.debug_voxel()
            m = _check(pkg, None, fused, 0.2, f"depth_window step {k}", t, got=got)
            np.testing.assert_array_equal(counts, m["counts"])
            np.testing.assert_array_equal(xyzi(got).view(np.uint32), W.depth_cloud.view(np.uint32))
    finally:
        d.lvo_set_centroid_mode(0)
    reg.close()
    t.done(500_000)
