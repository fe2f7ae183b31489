"""GPU tier: the global map (include/lvi_gmap.h) against its restatement (gmap_ref.py): fused clouds bit for bit, the
VoxelGrid's cells, counts and order exact and its centroids bit-equal to the model, PCL's overflow rule, the reservation,
no interference with the scan path (also with result / fetch on a second thread), and the host mirror's
publishGlobalMap and save_map."""
import threading

import numpy as np
import pytest

import gmap_ref as G
from helpers import bits, centroid_tol, small_params, xyzi

pytestmark = pytest.mark.gpu

N_KF = 40
KF_P = dict(max_keyframes=64, max_keyframe_points=600000)


@pytest.fixture(scope="module")
def kfs(pkg, oracle):
    """~40 keyframes (DS clouds in the sensor frame + pose) along the loop, made by the oracle"""
    S = pkg.synth
    o = pkg.LidarHotpath(oracle, **small_params())
    out = []
    for k in range(N_KF):
        pose = S.loop_pose(0.2 + 0.15 * k, 0.01 * np.sin(k), -0.01 * np.cos(k)).astype(np.float32)
        o.scan_upload(S.make_scan(16001, pose, 900 + k)); o.scan_organize(); o.scan_extract(); o.scan_downsample()
        c, s = o.get_scan_ds()
        out.append((c.copy(), s.copy(), pose))
    o.close()
    return out


@pytest.fixture(scope="module")
def ora(pkg, oracle):
    o = pkg.LidarHotpath(oracle, **small_params(max_map_points=1 << 21))
    yield o
    o.close()


def _store(pkg, hip, kfs, poses=None, **kw):
    h = pkg.LidarHotpath(hip, **small_params(**KF_P, **kw))
    for i, (c, s, p) in enumerate(kfs):
        h.keyframe_add(c, s, p if poses is None else poses[i])
    return h


def _check_case(pkg, ora, g, kfs, keys, which, leaf, poses, tag):
    corners, surfs = [k[0] for k in kfs], [k[1] for k in kfs]
    n = g.build(keys, which, leaf)
    r = g.result()
    fused_ref = G.fuse(ora, corners, surfs, poses, keys, which)
    assert n == r["n_fused"] == len(fused_ref), tag
    fused = g.fetch(pkg.gmap.FUSED)
    np.testing.assert_array_equal(bits(xyzi(fused)), bits(xyzi(fused_ref)), err_msg=tag)
    out = g.fetch(pkg.gmap.FILTERED)
    if leaf == 0:
        assert not r["filtered"] and r["n_out"] == n, tag
        np.testing.assert_array_equal(bits(xyzi(out)), bits(xyzi(fused_ref)), err_msg=tag)
        return r
    ref = G.voxel(pkg, ora, fused_ref, leaf)
    assert r["overflow"] == ref["overflow"], tag
    if ref["overflow"]:
        assert r["n_out"] == n, tag                                  # PCL: output = input, every point, in fuse order
        np.testing.assert_array_equal(bits(xyzi(out)), bits(xyzi(fused_ref)), err_msg=tag)
        assert len(g.debug_voxel()[0]) == 0
        return r
    cells, counts = g.debug_voxel()
    np.testing.assert_array_equal(cells, ref["cells"], err_msg=tag)
    np.testing.assert_array_equal(counts, ref["counts"], err_msg=tag)
    assert r["n_out"] == len(ref["cells"]) == len(out), tag
    np.testing.assert_array_equal(bits(xyzi(out)), bits(ref["pts"]), err_msg=tag)
    return r


def test_gmap_modes_and_leaves(pkg, hip, ora, kfs):
    """corner, surf and interleaved fuses of key lists with duplicates; leaf 0, 0.05 (filters on the hall), 0.02 (overflow rule)"""
    h = _store(pkg, hip, kfs)
    g = pkg.GlobalMap(h)
    g.reserve(1 << 20)
    poses = [k[2] for k in kfs]
    rng = np.random.default_rng(5)
    lists = [list(range(N_KF)), [3, 7, 7, 1, 39, 3, 20, 20, 0], list(rng.integers(0, N_KF, 30))]
    seen = set()
    for which in (G.CORNER, G.SURF, G.CORNER_SURF):
        for li, keys in enumerate(lists):
            for leaf in (0.0, 0.05, 0.02):
                r = _check_case(pkg, ora, g, kfs, keys, which, leaf, poses, f"which {which} list {li} leaf {leaf}")
                seen.add((leaf, r["overflow"]))
    assert (0.05, False) in seen and (0.02, True) in seen, seen
    h.close()


def test_gmap_overflow_at_shipped_leaf(pkg, hip, ora, kfs):
    """some poses 300 m away in x and y: the bbox overflows PCL's int32 cell count at 0.05, the result is the fused cloud"""
    poses = [k[2].copy() for k in kfs]
    for i in range(0, N_KF, 7):
        poses[i][3] += 300.0; poses[i][4] += 300.0
    h = _store(pkg, hip, kfs, poses)
    g = pkg.GlobalMap(h)
    g.reserve(1 << 20)
    for which in (G.CORNER, G.SURF, G.CORNER_SURF):
        r = _check_case(pkg, ora, g, kfs, [0, 1, 2, 7, 7, 14, 30], which, 0.05, poses, f"shifted which {which}")
        assert r["overflow"]
    h.close()


def test_gmap_pose_read_at_enqueue_and_errors(pkg, hip, ora, kfs):
    """a later keyframe_set_pose changes later builds only; bad arguments fail and leave the last result readable"""
    h = _store(pkg, hip, kfs)
    g = pkg.GlobalMap(h)
    with pytest.raises(pkg.LviError):
        g.build([0], G.CORNER_SURF, 0.05)                                # no reservation
    g.reserve(1 << 19)
    poses = [k[2].copy() for k in kfs]
    keys = [4, 5, 6]
    g.build(keys, G.CORNER_SURF, 0.0)
    moved = poses[5].copy(); moved[3] += 1.5
    h.keyframe_set_pose(5, moved)                                        # after the enqueue: not in this build
    fused = g.fetch(pkg.gmap.FUSED)
    ref = G.fuse(ora, [k[0] for k in kfs], [k[1] for k in kfs], poses, keys, G.CORNER_SURF)
    np.testing.assert_array_equal(bits(xyzi(fused)), bits(xyzi(ref)))
    poses[5] = moved
    _check_case(pkg, ora, g, kfs, keys, G.CORNER_SURF, 0.05, poses, "moved pose")
    before = g.result()
    out_before = g.fetch(pkg.gmap.FILTERED).copy()
    for args in (([0, N_KF], 2, 0.05), ([-1], 2, 0.05), ([0], 3, 0.05), ([0], 2, -0.05), ([0], 2, float("nan"))):
        with pytest.raises(pkg.LviError) as e:
            g.build(*args)
        assert e.value.code == -1, args
    assert g.result() == before
    np.testing.assert_array_equal(bits(xyzi(g.fetch(pkg.gmap.FILTERED))), bits(xyzi(out_before)))
    h.close()


def test_gmap_capacity(pkg, hip, ora, kfs):
    """a global map far above max_map_points (2^18): >= 1 M points exact; a build above the reservation fails with the state
    unchanged; at multi-million size cells and counts exact, centroids within centroid_tol of the mean"""
    h = _store(pkg, hip, kfs, max_map_points=1 << 18)
    g = pkg.GlobalMap(h)
    poses = [k[2] for k in kfs]
    per = sum(len(c) + len(s) for c, s, _ in kfs)
    rep_1m = -(-(1 << 20) // per)
    keys = list(range(N_KF)) * rep_1m
    g.reserve(len(keys) * per // N_KF + per)
    r = _check_case(pkg, ora, g, kfs, keys, G.CORNER_SURF, 0.05, poses, "1M")
    assert r["n_fused"] >= 1 << 20 and not r["overflow"]
    before = g.result()
    big = list(range(N_KF)) * (3 * rep_1m)
    with pytest.raises(pkg.LviError) as e:
        g.build(big, G.CORNER_SURF, 0.05)
    assert e.value.code == -4
    assert g.result() == before
    g.reserve(len(big) * per // N_KF + per)
    assert g.arena_bytes() > 0
    n = g.build(big, G.CORNER_SURF, 0.05)
    r = g.result()
    assert n >= 3 << 20 and not r["overflow"]
    fused = g.fetch(pkg.gmap.FUSED)
    ref = G.fuse(ora, [k[0] for k in kfs], [k[1] for k in kfs], poses, list(range(N_KF)), G.CORNER_SURF)
    np.testing.assert_array_equal(bits(xyzi(fused)), bits(np.tile(xyzi(ref), (3 * rep_1m, 1))))
    cells, counts = g.debug_voxel()
    rc, rn, mean = G.voxel_cells(fused, 0.05)
    np.testing.assert_array_equal(cells, rc)
    np.testing.assert_array_equal(counts, rn)
    out = xyzi(g.fetch(pkg.gmap.FILTERED))
    assert np.all(np.abs(out.astype(np.float64) - mean) <= centroid_tol(counts, out))
    h.close()


def test_gmap_fetch_windows(pkg, hip, ora, kfs):
    """windows of a fused cloud of at least three fetch chunks (65 536 points each): empty, one point, one short of / exactly /
    one past a chunk and two chunks, starts inside and on a chunk boundary, windows across boundaries, to the end — each
    bit-equal to the slice of the whole fetch; a window past the end fails with the result and the cloud unchanged"""
    CH = 65536
    h = _store(pkg, hip, kfs)
    g = pkg.GlobalMap(h)
    per = sum(len(c) + len(s) for c, s, _ in kfs)
    rep = -(-3 * CH // per)
    g.reserve(rep * per)
    N = g.build(list(range(N_KF)) * rep, G.CORNER_SURF, 0.0)
    assert N == rep * per >= 3 * CH
    before = g.result()
    ref = g.fetch(pkg.gmap.FUSED).copy()
    once = G.fuse(ora, [k[0] for k in kfs], [k[1] for k in kfs], [k[2] for k in kfs], list(range(N_KF)), G.CORNER_SURF)
    np.testing.assert_array_equal(bits(xyzi(ref)), bits(np.tile(xyzi(once), (rep, 1))))
    for first, count in ((0, 0), (0, 1), (0, CH - 1), (0, CH), (0, CH + 1), (1, CH), (CH - 1, 2), (CH - 1, CH + 1), (CH, CH), (0, 2 * CH),
                         (0, 2 * CH + 1), (7, N - 7), (N, 0)):
        got = g.fetch(pkg.gmap.FUSED, first, count)
        assert len(got) == count
        np.testing.assert_array_equal(bits(xyzi(got)), bits(xyzi(ref[first:first + count])), err_msg=f"first {first} count {count}")
    with pytest.raises(pkg.LviError) as e:
        g.fetch(pkg.gmap.FUSED, N - 1, 2)
    assert e.value.code == -1
    assert g.result() == before
    np.testing.assert_array_equal(bits(xyzi(g.fetch(pkg.gmap.FUSED))), bits(xyzi(ref)))
    h.close()


SEQ_P = dict(N_SCAN=4, Horizon_SCAN=8192, max_raw_points=20000, max_map_points=600000, max_keyframes=64, max_keyframe_points=600000)


def _seq_run(pkg, hip, scans, mode):
    """mode: None (no global map), 'build' (a build after every keyframe, result on this thread), 'thread' (result / fetch
    on a second thread while the next scans run)"""
    H = pkg.host_api
    m = H.SequentialMapper(pkg.load_host(), hip, pkg.default_params(hip, **SEQ_P), incremental_map=1)
    g = pkg.GlobalMap(m.handle) if mode else None
    if g:
        g.reserve(600000)
    rows, worker, got = [], None, []
    for k, sc in enumerate(scans):
        r = m.scan(sc, 20.0 + 0.2 * k)
        rows.append((bits(r["pose"]).copy(), [xyzi(c).view(np.uint32).copy() for c in m.handle.get_map_ds()] if k > 0 else None))
        if g and r["saved_keyframe"]:
            if worker is not None:
                worker.join()                                            # build may not overlap result / fetch
            n = g.build(list(range(r["n_keyframes"])), G.CORNER_SURF, 0.05)
            if mode == "build":
                got.append((n, g.result()["n_out"]))
            else:
                worker = threading.Thread(target=lambda n=n: got.append((n, g.result()["n_out"], len(g.fetch(pkg.gmap.FILTERED)))))
                worker.start()
    if worker is not None:
        worker.join()
    m.close()
    return rows, got


def test_gmap_no_interference(pkg, hip):
    """twin sequential runs: pose records and the local map bit-identical with and without a global-map build after every
    keyframe, and again with result / fetch on a second thread while the main thread runs scans"""
    S = pkg.synth
    n = 14
    poses = [S.loop_pose(0.3 + 0.05 * k, 0.004 * np.sin(k), -0.004 * np.cos(k)) for k in range(n)]
    scans = [S.make_scan(16001, poses[k], 3000 + k) for k in range(n)]
    base, _ = _seq_run(pkg, hip, scans, None)
    for mode in ("build", "thread"):
        rows, got = _seq_run(pkg, hip, scans, mode)
        assert len(got) >= 4, (mode, got)
        assert all(x[1] > 0 for x in got) and (mode == "build" or all(x[2] == x[1] for x in got)), got
        for k in range(n):
            np.testing.assert_array_equal(rows[k][0], base[k][0], err_msg=f"{mode} scan {k}")
            if k > 0:
                for x, y in zip(rows[k][1], base[k][1]):
                    np.testing.assert_array_equal(x, y, err_msg=f"{mode} scan {k}")


def _read_pcd(path):
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"DATA binary\n") + len(b"DATA binary\n")
    hdr = dict(line.split(" ", 1) for line in data[:end].decode().splitlines() if not line.startswith("#"))
    n = int(hdr["POINTS"])
    if hdr["FIELDS"] == "x y z intensity":
        return hdr, np.frombuffer(data[end:], np.float32).reshape(n, 4)
    dt = np.dtype([("f", np.float32, 7), ("t", np.float64)])
    return hdr, np.frombuffer(data[end:], dt, count=n)


def test_global_mapper_node(pkg, hip, oracle, ora, tmp_path):
    """after a 16-scan sequential run: publishGlobalMap = the restatement over that run's key poses and keyframe clouds;
    saveMap writes five files whose contents are the fused / filtered clouds and the key poses"""
    H, S = pkg.host_api, pkg.synth
    n = 16
    poses = [S.loop_pose(0.3 + 0.05 * k, 0.004 * np.sin(k), -0.004 * np.cos(k)) for k in range(n)]
    scans = [S.make_scan(16001, poses[k], 3000 + k) for k in range(n)]
    m = H.SequentialMapper(pkg.load_host(), hip, pkg.default_params(hip, **SEQ_P), incremental_map=1)
    gm = H.GlobalMapper(pkg.load_host(), m, 1000.0, 1.0, 0.05)
    gm.reserve(600000)
    assert gm.publishGlobalMap() is None                                   # no key poses yet
    corners, surfs = [], []
    for k, sc in enumerate(scans):
        r = m.scan(sc, 20.0 + 0.2 * k)
        if r["saved_keyframe"]:
            c, s = m.handle.get_scan_ds()                                  # what keyframe_add_current copied
            corners.append(c.copy()); surfs.append(s.copy())
    kp = m.keyposes()                                                      # x y z roll pitch yaw time intensity
    assert len(kp) == len(corners) >= 5
    pose6 = [np.array([p[3], p[4], p[5], p[0], p[1], p[2]], np.float32) for p in kp]
    p3 = kp[:, [0, 1, 2, 7]].astype(np.float32)

    def vf(pts, leaf):
        return xyzi(ora.voxel_downsample(np.ascontiguousarray(pts, np.float32).view(pkg.PT_DTYPE).reshape(-1), leaf))
    keys = G.select_keys(p3, 1000.0, 1.0, vf)
    np.testing.assert_array_equal(gm.keys(), keys)
    cloud, info = gm.publishGlobalMap()
    fused = G.fuse(ora, corners, surfs, pose6, keys, G.CORNER_SURF)
    assert info["n_fused"] == len(fused)
    ref = G.voxel(pkg, ora, fused, 0.05)
    np.testing.assert_array_equal(bits(xyzi(cloud)), bits(ref["pts"]))
    for res in (0.0, 0.4):
        d = tmp_path / f"map_{res}"
        assert gm.saveMap(str(d), res)
        allk = list(range(len(kp)))
        raw = [G.fuse(ora, corners, surfs, pose6, allk, w) for w in (G.CORNER, G.SURF)]
        for name, w in (("CornerMap.pcd", 0), ("SurfMap.pcd", 1)):
            hdr, pts = _read_pcd(d / name)
            exp = xyzi(raw[w]) if res == 0 else G.voxel(pkg, ora, raw[w], res)["pts"]
            np.testing.assert_array_equal(bits(pts), bits(exp), err_msg=name)
        _, gl = _read_pcd(d / "GlobalMap.pcd")
        np.testing.assert_array_equal(bits(gl), bits(np.concatenate([xyzi(raw[0]), xyzi(raw[1])])))
        _, tr = _read_pcd(d / "trajectory.pcd")
        np.testing.assert_array_equal(bits(tr), bits(p3))
        hdr, tf = _read_pcd(d / "transformations.pcd")
        assert hdr["SIZE"] == "4 4 4 4 4 4 4 8" and len(tf) == len(kp)
        np.testing.assert_array_equal(tf["f"][:, :4], p3)
        np.testing.assert_array_equal(tf["f"][:, 4:], kp[:, 3:6].astype(np.float32))
        np.testing.assert_array_equal(tf["t"], kp[:, 6])
    gm.close()
    m.close()


HAND_CASES = [
    # (key positions, radius, pose density, expected key list): distance ties (VoxelGrid order, not search order)
    ([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 0)], 1000.0, 0.1, [3, 1, 4, 0, 2]),
    # a DS centroid equidistant from two keys: the first index
    ([(0.25, 0, 0), (0.75, 0, 0), (5.5, 0, 0)], 1000.0, 1.0, [0, 2]),
    # the centroid of voxel (0,0,0) is nearer to the key of voxel (1,0,0): that key is fused twice
    ([(0.0, 0.0, 0.0), (0.9, 0.9, 0.0), (1.0, 0.45, 0.0)], 1000.0, 1.0, [2, 2]),
    # keys beyond R of back() are not searched
    ([(0.5, 0.5, 0.5), (30.0, 0, 0), (9.5, 0, 0), (10.5, 0, 0), (0, 0, 0)], 10.0, 0.5, [4, 2, 0]),
    # one 20 m voxel holds keys 0, 2, 4: its centroid names key 0 once
    ([(0.5, 0.5, 0.5), (30.0, 0, 0), (9.5, 0, 0), (10.5, 0, 0), (0, 0, 0)], 10.0, 20.0, [0]),
]


def test_global_mapper_keys_hand_cases(pkg, hip, ora):
    """GlobalMapper::globalMapKeys (keyPosesWithin, downsampleKeyPoses, assignNearestKeys) on the hand cases of the restatement:
    ties, a key fused twice, the radius cut; equal to the expected lists and to gmap_ref.select_keys"""
    H = pkg.host_api
    c = np.zeros(4, pkg.PT_DTYPE)
    for i in range(4):
        c[i] = (0.1 * i, 0.2, 0.3, 1.0)

    def vf(pts, leaf):
        return xyzi(ora.voxel_downsample(np.ascontiguousarray(pts, np.float32).view(pkg.PT_DTYPE).reshape(-1), float(leaf)))
    for xyz, radius, density, expected in HAND_CASES:
        m = H.SequentialMapper(pkg.load_host(), hip, pkg.default_params(hip, **SEQ_P), incremental_map=1)
        gm = H.GlobalMapper(pkg.load_host(), m, radius, density, 0.05)
        for i, p in enumerate(xyz):
            m.seed_keyframe(c, c, [0.0, 0.0, 0.0, p[0], p[1], p[2]], 10.0 + i)
        got = gm.keys()
        np.testing.assert_array_equal(got, expected, err_msg=str(xyz))
        p3 = np.zeros((len(xyz), 4), np.float32)
        p3[:, :3] = np.asarray(xyz, np.float32); p3[:, 3] = np.arange(len(xyz))
        np.testing.assert_array_equal(got, G.select_keys(p3, radius, density, vf))
        gm.reserve(64)
        cloud, info = gm.publishGlobalMap()
        assert info["n_fused"] == 8 * len(expected)
        gm.close(); m.close()


def test_gmap_small_reservation(pkg, hip, kfs):
    """a reservation below the arena's minimum size still bounds the fused cloud"""
    h = _store(pkg, hip, kfs[:2])
    g = pkg.GlobalMap(h)
    g.reserve(10)
    with pytest.raises(pkg.LviError) as e:
        g.build([0], G.CORNER, 0.0)                         # a keyframe's corner cloud holds more than 10 points
    assert e.value.code == -4
    h.close()
