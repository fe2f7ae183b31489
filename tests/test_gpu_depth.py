"""GPU tier: the LiDAR depth association (include/lvi_depth.h, csrc/lvi_depth.hip) against its numpy restatement
(tests/depth_ref.py): range image, depths, the band-limited search, the cloud window, the node's depth channel, a full
size scene and the error paths."""
import math

import numpy as np
import pytest

import depth_ref as R

pytestmark = pytest.mark.gpu

BOUNDARY_TOL = 1e-4          # bins: a point whose row / column value lies this close to k + 0.5 may round either way


def _xyzi(pkg, a):
    return pkg._abi.pts_xyzi(a).copy() if len(a) else np.zeros((0, 4), np.float32)


def _shell(n, seed, rmin=6.0, rmax=14.0, max_el=85.0):
    """points in front of the body over a wide solid angle (elevations up to max_el degrees)"""
    rng = np.random.default_rng(seed)
    az = np.deg2rad(rng.uniform(-80, 80, n)); el = np.deg2rad(rng.uniform(-max_el, max_el, n))
    r = rmin + (rmax - rmin) * (0.5 + 0.5 * np.sin(2 * az) * np.cos(el))          # a smooth surface: neighbours within 2 m
    p = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), rng.uniform(0, 100, n)], 1)
    return p.astype(np.float32)


def _wall(n, seed, x0=9.0):
    rng = np.random.default_rng(seed)
    p = np.stack([x0 + rng.normal(0, 0.3, n), rng.uniform(-8, 8, n), rng.uniform(-6, 6, n), rng.uniform(0, 100, n)], 1)
    return p.astype(np.float32)


def _features(n, seed, u=0.6, v=0.45):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-u, u, n), rng.uniform(-v, v, n), np.ones(n)], 1).astype(np.float32)


def _boundary_bins(local):
    """bins any point could land in when its row / column value is within BOUNDARY_TOL of a rounding boundary"""
    x, y, z = (local[:, k].astype(np.float64) for k in range(3))
    rr = (np.arctan2(z, np.sqrt(x * x + y * y)) * 180.0 / math.pi + 90.0) / 0.5
    cc = (np.arctan2(x, y) * 180.0 / math.pi) / 0.5
    near = (np.abs(rr - np.floor(rr) - 0.5) < BOUNDARY_TOL) | (np.abs(cc - np.floor(cc) - 0.5) < BOUNDARY_TOL)
    bins = set()
    for i in np.nonzero(near)[0]:
        for r in (math.floor(rr[i]), math.ceil(rr[i])):
            for c in (math.floor(cc[i]), math.ceil(cc[i])):
                bins.add((r, c))
    return bins


def _compare(pkg, oracle, reg, cloud, pose6, feats, min_agree=0.99):
    """one get_depth on both sides from the same depth cloud: range image (up to rounding-boundary points), sphere cloud,
    the search against the exhaustive one on the device's sphere cloud (exact), neighbours and depths against the kd-tree's
    (bit-equal wherever the neighbours agree).  Returns (gpu depths, ref depths, agreement)."""
    d_gpu = reg.get_depth(pose6, feats)
    d_ref, dbg = R.get_depth(oracle, cloud, pose6, feats)
    if len(feats) == 0:
        assert len(d_gpu) == 0
        return d_gpu, d_ref, 1.0
    sel_gpu = reg.debug_range()
    diff = np.argwhere(sel_gpu != dbg["sel"])
    allowed = _boundary_bins(dbg["local"])
    unexplained = [tuple(b) for b in diff if tuple(b) not in allowed]
    assert not unexplained, f"{len(unexplained)} range-image bins differ without a rounding-boundary point: {unexplained[:5]}"
    sph = _xyzi(pkg, reg.debug_sphere())
    assert len(sph) == len(dbg["sphere"])
    if len(diff) == 0:
        assert np.array_equal(sph.view(np.uint32), dbg["sphere"].view(np.uint32))
    if "nbr" not in dbg:
        assert (d_gpu == -1).all()
        return d_gpu, d_ref, 1.0
    nbr_gpu, sqd_gpu = reg.debug_neighbors()
    # the search itself has no allowance: on the device's own sphere cloud it is the exhaustive 3-NN, in either mode, and
    # every accepted feature's depth is the plane intersection of the device's own neighbours
    R.check_search(sph, dbg["V"], nbr_gpu, sqd_gpu, d_gpu, full=False)
    reg.set_full_search(True)
    try:
        d_full = reg.get_depth(pose6, feats)
        R.check_search(_xyzi(pkg, reg.debug_sphere()), dbg["V"], *reg.debug_neighbors(), d_full, full=True)
    finally:
        reg.set_full_search(False)
    assert np.array_equal(d_full.view(np.uint32), d_gpu.view(np.uint32))
    # where neither side accepts its 3rd neighbour, the band's neighbours need not be the global ones: both publish -1
    acc = ((nbr_gpu >= 0).all(1) & (sqd_gpu[:, 2] < R.DIST_SQ_THRESHOLD)) | ((dbg["nbr"] >= 0).all(1) & (dbg["sqd"][:, 2] < R.DIST_SQ_THRESHOLD))
    assert (d_gpu[~acc] == -1).all() and (d_ref[~acc] == -1).all()
    same = acc & (nbr_gpu == dbg["nbr"]).all(1)
    assert np.array_equal(d_gpu[same].view(np.uint32), d_ref[same].view(np.uint32)), np.nonzero(d_gpu[same] != d_ref[same])
    assert np.array_equal(sqd_gpu[same].view(np.uint32), dbg["sqd"][same].view(np.uint32))
    agree = same.sum() / max(acc.sum(), 1)
    assert agree >= min_agree, (agree, int(acc.sum()))
    return d_gpu, d_ref, agree


def test_range_image_and_depths_on_identical_input(pkg, oracle, hip):
    reg = pkg.DepthRegister(hip, max_clouds=4, max_cloud_points=200000, max_features=150, lidar_skip=0)
    pose = (1.0, -0.5, 0.2, 0.05, -0.03, 0.4)
    M = R.get_transformation(oracle, pose)
    local = _shell(150000, 3)
    cloud = R.transform(M, local)                                   # a world-frame cloud the body at `pose` sees as `local`
    reg.set_cloud(cloud)
    assert np.array_equal(_xyzi(pkg, reg.get_cloud()).view(np.uint32), cloud.view(np.uint32))
    # features over the image, plus high elevations (|z/x| near 10) and a feature at the band's edge
    f = _features(150, 5)
    f[:10, 1] = np.linspace(-9.9, 9.9, 10)
    d, dr, agree = _compare(pkg, oracle, reg, cloud, pose, f)
    assert (d > 0).mean() > 0.5, (d > 0).mean()
    _compare(pkg, oracle, reg, cloud, pose, f[:0])                  # 0 features
    _compare(pkg, oracle, reg, cloud, pose, f[:1])
    print(f"range image / depths: neighbour agreement {agree:.4f}, {int((d > 0).sum())} of 150 with depth")


def test_band_search_equals_unrestricted_search(pkg, oracle, hip):
    reg = pkg.DepthRegister(hip, max_clouds=2, max_cloud_points=200000, max_features=4096, lidar_skip=0)
    pose = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    cloud = _shell(120000, 11)
    reg.set_cloud(cloud)
    f = _features(4000, 12, u=3.0, v=10.0)
    d_band = reg.get_depth(pose, f)
    n_band, s_band = reg.debug_neighbors()
    reg.set_full_search(True)
    d_full = reg.get_depth(pose, f)
    n_full, s_full = reg.debug_neighbors()
    reg.set_full_search(False)
    assert np.array_equal(d_band.view(np.uint32), d_full.view(np.uint32))
    acc = s_full[:, 2] < R.DIST_SQ_THRESHOLD
    assert acc.mean() > 0.3, acc.mean()
    assert np.array_equal(n_band[acc], n_full[acc]) and np.array_equal(s_band[acc].view(np.uint32), s_full[acc].view(np.uint32))
    assert not (s_band[~acc, 2] < R.DIST_SQ_THRESHOLD).any()        # the band never accepts what the full search rejects
    print(f"band vs full: {len(f)} features, {int(acc.sum())} accepted, identical")


def test_window_maintenance(pkg, oracle, hip):
    skip = 2
    reg = pkg.DepthRegister(hip, max_clouds=12, max_cloud_points=30000, max_features=150, lidar_skip=skip)
    W = R.Window(pkg, oracle, lidar_skip=skip, window_s=5.0)
    for k in range(36):
        stamp = 100.0 + 0.25 * k
        pose = None if k == 9 else (0.3 * k * 0.25, 0.05 * k * 0.25, 0.0, 0.0, 0.01 * k, 0.02 * k)
        cloud = _wall(20000, 100 + k)
        u_gpu = reg.lidar_callback(cloud, pose, stamp)
        u_ref = W.lidar_callback(cloud, pose, stamp)
        assert u_gpu == u_ref, k
        st = reg.state()
        assert st["n_clouds"] == len(W.stamps) and st["lidar_count"] == W.lidar_count, (k, st)
        if not u_gpu:
            continue
        dc = _xyzi(pkg, reg.get_cloud())
        assert len(dc) == len(W.depth_cloud), k
        cells, counts = reg.debug_voxel()
        assert np.array_equal(cells, W.cells) and np.array_equal(counts, W.counts), k
        np.testing.assert_allclose(dc, W.depth_cloud, rtol=0, atol=1e-4)
    assert reg.state()["used_total"] == 11
    print(f"window: 36 callbacks, {reg.state()}")


def test_node_depth_channel(pkg, oracle, hip):
    from test_host_nodes import CAM
    H = pkg.host_api
    hl = pkg.load_host()
    w, h = 240, 180
    tp = pkg.default_tracker_params(hip, max_width=w, max_height=h, max_cnt=60, min_dist=12.0)
    node = H.TrackerNode(hl, tp, h, w, 10, equalize=False, cam=CAM)
    nd = H.NodeDepthRegister(hl, node, hip, max_clouds=32, max_cloud_points=30000, max_features=int(tp.max_features), lidar_skip=1)
    S = pkg.synth
    img0 = S.make_texture(w, h, 9)
    frames = [img0] + [S.warp_homography(img0, S.small_motion_homography(w, h, 10 + i, 2.0)) for i in range(7)]
    pose_at = lambda t: (0.2 * (t - 50.0), 0.02 * (t - 50.0), 0.0, 0.0, 0.0, 0.01 * (t - 50.0))  # noqa: E731
    W = R.Window(pkg, oracle, lidar_skip=1, window_s=5.0)
    checked = with_depth = total = 0
    worst = 1.0
    for k in range(48):
        t = 50.0 + 0.1 * k
        cloud = _wall(20000, 500 + k)                             # sensor frame, 10 Hz, every second one used
        assert nd.lidar_callback(cloud, pose_at(t), t) == W.lidar_callback(cloud, pose_at(t), t)
        nd.set_image_pose(pose_at(t + 0.05))
        r = node.image(frames[k % len(frames)], t + 0.05)
        if r["outcome"] not in ("published", "first_publish_suppressed") or len(r["points"]) == 0:
            continue
        ch5 = r["channels"][5]
        dc = _xyzi(pkg, nd.register.get_cloud())
        d_ref, dbg = R.get_depth(oracle, dc, pose_at(t + 0.05), r["points"])
        nbr_gpu, sqd_gpu = nd.register.debug_neighbors()
        sph = _xyzi(pkg, nd.register.debug_sphere())
        if len(sph) >= 10:                                         # the search is exact on the device's own sphere cloud
            R.check_search(sph, R.feature_rays(r["points"]), nbr_gpu, sqd_gpu, np.ascontiguousarray(ch5, np.float32), full=False)
        same = (nbr_gpu == dbg["nbr"]).all(1) if "nbr" in dbg else np.ones(len(ch5), bool)
        same |= (ch5 == -1) & (d_ref == -1)                        # both reject: the band's far neighbours need not be the global ones
        assert np.array_equal(ch5[same].view(np.uint32), d_ref[same].view(np.uint32)), k
        assert same.mean() >= 0.99, (k, same.mean())
        worst = min(worst, same.mean())
        checked += 1
        with_depth += int((ch5 > 0).sum()); total += len(ch5)
    assert checked >= 40, checked
    assert with_depth >= 0.3 * total, (with_depth, total)
    print(f"node: {checked} messages, {with_depth} of {total} features with depth, lowest kd-tree agreement {worst:.4f}")
    nd.close(); node.close()


def test_full_size_scene(pkg, oracle, hip):
    S = pkg.synth
    n_raw = 100001
    reg = pkg.DepthRegister(hip, max_clouds=16, max_cloud_points=n_raw, max_features=150, lidar_skip=0)
    W = R.Window(pkg, oracle, lidar_skip=0, window_s=5.0)
    for k in range(12):
        p = S.loop_pose(0.03 * k)                                  # (roll, pitch, yaw, x, y, z) of the sensor
        scan = S.make_scan(n_raw, p, 40 + k)
        cloud = np.stack([scan["x"], scan["y"], scan["z"], scan["reflectivity"].astype(np.float32)], 1).astype(np.float32)
        pose6 = (p[3], p[4], p[5], p[0], p[1], p[2])
        assert reg.lidar_callback(cloud, pose6, 10.0 + 0.1 * k) and W.lidar_callback(cloud, pose6, 10.0 + 0.1 * k)
    dc = _xyzi(pkg, reg.get_cloud())
    cells, counts = reg.debug_voxel()
    assert np.array_equal(cells, W.cells) and np.array_equal(counts, W.counts)
    f = _features(150, 77)
    d, dr, agree = _compare(pkg, oracle, reg, dc, pose6, f)
    print(f"full size: depth cloud {len(dc)} points, neighbour agreement {agree:.4f}, {int((d > 0).sum())} of 150 with depth")


def test_errors(pkg, hip):
    A = pkg._abi
    reg = pkg.DepthRegister(hip, max_clouds=2, max_cloud_points=1000, max_features=8, lidar_skip=0)
    with pytest.raises(pkg.LviError) as e:
        reg.lidar_callback(_wall(1001, 1), (0,) * 6, 0.0)
    assert e.value.code == A.LVI_ERR_CAPACITY and reg.state()["lidar_count"] == -1
    assert reg.lidar_callback(_wall(1000, 2), (0,) * 6, 0.0) and reg.lidar_callback(_wall(1000, 3), (0,) * 6, 1.0)
    with pytest.raises(pkg.LviError) as e:
        reg.lidar_callback(_wall(1000, 4), (0,) * 6, 2.0)            # a third cloud inside 5 s
    assert e.value.code == A.LVI_ERR_CAPACITY and reg.state()["n_clouds"] == 2
    with pytest.raises(pkg.LviError) as e:
        reg.get_depth((0,) * 6, _features(9, 1))
    assert e.value.code == A.LVI_ERR_CAPACITY
    f = _features(8, 2)
    reg.get_depth((0,) * 6, f)
    sel, sph = reg.debug_range(), reg.debug_sphere()
    assert (reg.get_depth(None, f) == -1).all()                     # no transform: -1, the device state untouched
    assert np.array_equal(reg.debug_range(), sel) and np.array_equal(reg.debug_sphere(), sph)
    reg.close()
