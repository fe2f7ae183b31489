"""GPU tier: the LiDAR depth association (csrc/lvi_depth.hip) at its branches, ties, smallest shapes and block edges.
Hand-built scenes (tests/depth_scenes.py, checked on the CPU by tests/test_depth_scenes.py) in band and in full-search
mode against the numpy restatement (tests/depth_ref.py), with no allowance: range image, sphere cloud, neighbours,
distances and depths are exact.  Then the cloud window at its block edges, with empty and fully cut clouds, through the
host and the device entry."""
import ctypes as C

import numpy as np
import pytest

import depth_ref as R
import depth_scenes as S

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("full", [False, True], ids=["band", "full_search"])


def _xyzi(pkg, a):
    return pkg._abi.pts_xyzi(a).copy() if len(a) else np.zeros((0, 4), np.float32)


@pytest.fixture(scope="module")
def reg(pkg, hip):
    r = pkg.DepthRegister(hip, max_clouds=1, max_cloud_points=4096, max_features=150, lidar_skip=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def ref(oracle):
    """the restatement of one scene, computed once: name -> (world cloud, ref depths, debug dict)"""
    cache = {}

    def get(name, body_cloud, pose, feats):
        if name not in cache:
            world = R.transform(R.get_transformation(oracle, pose), body_cloud)
            cache[name] = (world,) + R.get_depth(oracle, world, pose, feats)
        return cache[name]
    return get


def _exact(pkg, reg, ref, name, body_cloud, pose, feats, full):
    """one get_depth of a scene: everything the device computed equals the restatement and the exhaustive search.
    Returns (depths, sphere, neighbours, distances, debug dict of the restatement, its depths)."""
    world, d_ref, dbg = ref(name, body_cloud, pose, feats)
    reg.set_cloud(world)
    reg.set_full_search(full)
    try:
        d = reg.get_depth(pose, feats)
    finally:
        reg.set_full_search(False)
    assert np.array_equal(reg.debug_range(), dbg["sel"]), name
    sph = _xyzi(pkg, reg.debug_sphere())
    assert np.array_equal(sph.view(np.uint32), dbg["sphere"].view(np.uint32)), name
    nbr, sqd = reg.debug_neighbors()
    assert nbr.shape == (len(feats), 3) and sqd.shape == (len(feats), 3)
    if len(sph) < 10:
        assert "nbr" not in dbg and (d == -1).all() and (nbr == -1).all() and (sqd == -1).all(), name
    else:
        R.check_search(sph, dbg["V"], nbr, sqd, d, full)
        acc = R.accepted(nbr, sqd) | R.accepted(dbg["nbr"], dbg["sqd"])
        if full:
            acc[:] = True
        assert np.array_equal(nbr[acc], dbg["nbr"][acc]) and np.array_equal(sqd[acc].view(np.uint32), dbg["sqd"][acc].view(np.uint32)), name
    assert np.array_equal(d.view(np.uint32), d_ref.view(np.uint32)), (name, np.nonzero(d != d_ref)[0][:5])
    return d, sph, nbr, sqd, dbg, d_ref


# ---------------------------------------------------------------------------------------------------------- scenes
@MODES
@pytest.mark.parametrize("pose", [S.IDENT, S.POSE2], ids=["identity", "posed"])
def test_branches(pkg, reg, ref, pose, full):
    """every branch of the plane intersection, 15 features each, exactly max_features features in one call"""
    cloud, feats, labels, own = S.branches()
    assert len(feats) == reg.max_features
    d, sph, nbr, sqd, dbg, d_ref = _exact(pkg, reg, ref, f"branches{pose}", cloud, pose, feats, full)
    counts, taken = S.class_counts(labels, own, dbg["sphere_idx"], sph, nbr, sqd, dbg["V"], d)
    want, _ = S.class_counts(labels, own, dbg["sphere_idx"], dbg["sphere"], dbg["nbr"], dbg["sqd"], dbg["V"], d_ref)
    print(f"branches pose={pose} full={full}: {counts}; collinear features took {sorted(t for t, c in zip(taken, labels) if c == 'collinear')}")
    assert counts == want and all(counts[c] >= 10 for c in S.CLASSES), (counts, want)


@MODES
def test_ties(pkg, reg, ref, full):
    """bit-equal distances: the range image keeps the lower cloud index, the 3-NN puts the lower sphere index first and
    keeps it when the tie is for the last place"""
    clouds = S.ties()
    out = {name: _exact(pkg, reg, ref, f"ties_{name}", c, S.IDENT, S.AXIS_FEATURE, full) for name, c in clouds.items()}
    for name in clouds:
        d, sph, nbr, sqd, dbg, _ = out[name]
        v = dbg["V"][0]
        dx, dy, dz = (v[k] - sph[:, k] for k in range(3))
        dist = ((dx * dx + dy * dy) + dz * dz).view(np.uint32)
        bits = sqd[0].view(np.uint32)
        for place in range(3):                                   # each place holds the lowest index not yet taken at its distance
            tied = [j for j in np.nonzero(dist == bits[place])[0] if j not in nbr[0, :place]]
            assert nbr[0, place] == min(tied), (name, place, nbr[0], tied)
        assert R.accepted(nbr, sqd)[0] and d[0] > 3, name
    b = out["pairs"][3][0].view(np.uint32)
    assert b[0] == b[1] and (out["pairs"][2][0, :2] == (6, 7)).all()
    b = out["single_then_pair"][3][0].view(np.uint32)
    assert b[0] < b[1] == b[2]
    sel = out["repeated"][4]["sel"]                              # equal to the device's: _exact has compared them
    assert (sel == 0).sum() == 1 and (sel == 3).sum() == 0 and sel.max() == len(clouds["repeated"]) - 1
    assert np.array_equal(out["repeated"][0].view(np.uint32), out["pairs"][0].view(np.uint32))


@MODES
def test_small(pkg, reg, ref, full):
    """fewer than ten sphere entries give -1 without a search, ten search; the origin's NaN entry is counted and never a
    neighbour; the field-of-view ratio of exactly 10 is kept"""
    for name, cloud in S.small().items():
        d, sph, nbr, sqd, dbg, _ = _exact(pkg, reg, ref, f"small_{name}", cloud, S.IDENT, S.SMALL_FEATURES, full)
        nsph, searched = S.SMALL_EXPECT[name]
        assert len(sph) == nsph, name
        if searched:
            assert (nbr >= 0).all() and (sqd >= 0).all(), name
        else:
            assert (d == -1).all() and (nbr == -1).all(), name
        nan = np.nonzero(np.isnan(sph[:, :3]).any(1))[0]
        if name.startswith("origin"):
            assert len(nan) == 1 and sph[nan[0], 3] == 0 and not np.isin(nbr, nan).any(), name
        else:
            assert len(nan) == 0, name
        if name in ("ten_bins", "origin_plus_10", "x_zero", "ratio_ten"):
            assert (d[:2] > 3).all(), (name, d)
    sel = reg.debug_range()                                       # ratio_ten is the last scene
    assert set(sel[sel >= 0]) == set(range(14))
    # an empty depth cloud: -1 for every feature, nothing searched
    reg.set_cloud(np.zeros((0, 4), np.float32))
    assert (reg.get_depth(S.IDENT, S.SMALL_FEATURES) == -1).all() and reg.state()["n_depth_cloud"] == 0
    assert len(reg.debug_neighbors()[0]) == 0
    with pytest.raises(pkg.LviError):
        reg.debug_range()


@MODES
def test_features(pkg, reg, ref, full):
    """the zero vector, bands clipped at rows 0 and 359 (with and without neighbours inside the acceptance arc), a feature
    looking backwards, and a call with one feature"""
    cloud, f = S.features()
    d, sph, nbr, sqd, dbg, _ = _exact(pkg, reg, ref, "features", cloud, S.IDENT, f, full)
    assert R.accepted(nbr, sqd).tolist() == [False, False, False, True, True, True, False]
    assert (d[3:6] > 3).all() and (d[[0, 1, 2, 6]] == -1).all()
    d1, _, nbr1, _, _, _ = _exact(pkg, reg, ref, "features_one", cloud, S.IDENT, f[3:4], full)
    assert d1[0].view(np.uint32) == d[3].view(np.uint32) and np.array_equal(nbr1[0], nbr[3])


def test_wall_gives_the_analytic_depth(pkg, oracle, reg):
    """independent of the restatement: a feature (u, v, 1) meets the wall x = 10 at depth 10"""
    from test_depth_cpu import _plane_cloud
    cloud = _plane_cloud(10.0, step=0.146)
    assert len(cloud) == 3025
    feats = np.array([[0.0, 0.0, 1.0], [0.05, -0.03, 1.0], [-0.1, 0.08, 1.0]], np.float32)
    reg.set_cloud(cloud)
    d = reg.get_depth(S.IDENT, feats)
    print("wall:", d - 10.0)
    assert np.all(np.abs(d - 10.0) < 1e-3), d


# ---------------------------------------------------------------------------------------------------------- window
def _device_copy(rt, a):
    a = np.ascontiguousarray(a)
    p = C.c_void_p()
    assert rt.hipMalloc(C.byref(p), max(a.nbytes, 16)) == 0
    if a.nbytes:
        assert rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
    return p


def test_window_at_block_edges(pkg, oracle, hip):
    """clouds of 0, 1, 1023, 1024, 1025, 2049, 0, 3000 (all cut) and 7 points, half of each cut by the field of view, in a
    window of three slots that pops at every callback from the fourth on: empty slots at the front, in the middle and at
    the back, every slot reused.  Host entry against the restatement, device entry against the host entry."""
    rt = C.CDLL("libamdhip64.so.7")                              # the runtime liblvi_hip.so is linked against
    rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipFree.argtypes = [C.c_void_p]
    kw = dict(max_clouds=3, max_cloud_points=3000, max_features=8, lidar_skip=0, window_s=1.0)
    host, dev = pkg.DepthRegister(hip, **kw), pkg.DepthRegister(hip, **kw)
    W = R.Window(pkg, oracle, lidar_skip=0, window_s=1.0)
    sizes = []
    for k, cloud in enumerate(S.window_sequence()):
        pose, stamp = S.window_pose(k), S.window_stamp(k)
        d_cloud = _device_copy(rt, cloud)
        try:
            u_dev = dev.lidar_callback_device(d_cloud.value, len(cloud), pose, stamp)
        finally:
            assert rt.hipFree(d_cloud) == 0
        u_host = host.lidar_callback(cloud, pose, stamp)
        assert u_host and u_dev and W.lidar_callback(cloud, pose, stamp), k
        sizes.append([len(c) for c in W.clouds])
        assert sizes[-1][-1] == S.WINDOW_KEPT[k], k
        st = host.state()
        assert st["n_clouds"] == len(W.stamps) and st["lidar_count"] == W.lidar_count and st["used_total"] == k + 1, (k, st)
        assert dev.state() == st, k
        dc = _xyzi(pkg, host.get_cloud())
        assert len(dc) == len(W.depth_cloud) == st["n_depth_cloud"], k
        cells, counts = host.debug_voxel()
        assert np.array_equal(cells, W.cells) and np.array_equal(counts, W.counts), k
        np.testing.assert_allclose(dc, W.depth_cloud, rtol=0, atol=1e-4)
        assert np.array_equal(_xyzi(pkg, dev.get_cloud()).view(np.uint32), dc.view(np.uint32)), k
        if len(dc) == 0:                                         # an empty depth cloud: get_depth publishes -1
            assert (host.get_depth(pose, S.SMALL_FEATURES) == -1).all(), k
    assert sizes[0] == [0] and sizes[6] == [513, 1025, 0] and sizes[7] == [1025, 0, 0] and sizes[8] == [0, 0, 4]
    print(f"window edges: {sizes}")
    host.close(); dev.close()
