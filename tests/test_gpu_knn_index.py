"""GPU tier (-m gpu): the KNN grid index of the downsampled local map, through every producer of its count step.

The index is built in two launches after a binned map rebuild (the count is taken inside vb_copy/map, the chunk totals of the
cell scan where the counts are taken) and in three after every other producer (sorted realisation, incremental map).  Every
expectation here is exhaustive search in numpy over the library's own lvi_get_map_ds clouds: the five nearest by the
(squared distance, index) order the kernels document, distances as ((dx*dx)+dy*dy)+dz*dz in f32, entries at 1 m or more
reported as (-1, inf).  Neighbours and squared distances must match bit for bit; nothing is tolerated.

The map shapes are the smallest that reach each path of the build: fewer cells than scan chunks (one cell per chunk), a cell
count that is no multiple of the chunks, 1 m cells, an empty segment, PCL's overflow rule (output = input, counted in
vb_copy's other branch), and a small map built right after a large one on the same handle (the chunk totals must start
from zero again)."""
import numpy as np
import pytest

from helpers import bits, make_small_scene, small_params, xyzi

pytestmark = pytest.mark.gpu

GRID_SCAN_BLOCKS = 1024
SMALL = dict(max_map_points=40000)                       # the smallest cell budget: 2^18 cells


def _max_cells(max_map_points):
    return min(1 << 24, max(1 << 18, 4 * max(max_map_points, 64)))


def _geometry(raw, max_map_points):
    """grid_meta_one restated: (cells per axis, cell edge in half metres) for a raw map segment"""
    p = xyzi(raw)[:, :3].astype(np.float64)
    mn, mx = np.floor(p.min(axis=0)), np.floor(p.max(axis=0))
    ext = mx - mn + 3.0
    c = 1
    while True:
        dim = np.ceil(ext / (0.5 * c))
        if dim.prod() <= _max_cells(max_map_points):
            return dim.astype(np.int64), c
        c += 1


def _brute_knn(m, q):
    m, q = xyzi(m), xyzi(q)
    n, nq = len(m), len(q)
    idx = np.full((nq, 5), -1, np.int32)
    sqd = np.full((nq, 5), np.inf, np.float32)
    if n == 0:
        return idx, sqd
    ids = np.arange(n, dtype=np.uint64)[None, :]
    k = min(5, n)
    for s in range(0, nq, 256):
        qq = q[s:s + 256]
        ex, ey, ez = (qq[:, None, a] - m[None, :, a] for a in range(3))
        d = np.ascontiguousarray((ex * ex + ey * ey) + ez * ez, np.float32)
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids       # squared distances are >= 0: their bits order like integers
        best = np.sort(np.partition(key, k - 1, axis=1)[:, :k], axis=1)
        dd = (best >> np.uint64(32)).astype(np.uint32).view(np.float32)
        ii = (best & np.uint64(0xFFFFFFFF)).astype(np.int32)
        ok = dd < np.float32(1.0)
        idx[s:s + len(qq), :k] = np.where(ok, ii, -1)
        sqd[s:s + len(qq), :k] = np.where(ok, dd, np.float32(np.inf))
    return idx, sqd


def _queries(rng, m, nq=1200):
    """map points as they are (distance 0), jittered ones (dense neighbourhoods, some with fewer than five within 1 m), far ones"""
    m = xyzi(m)
    q = np.zeros((nq, 4), np.float32)
    if len(m) == 0:
        q[:, :3] = rng.uniform(-5, 5, (nq, 3))
        return q
    q[:] = m[rng.integers(0, len(m), nq)]
    q[100:, :3] += rng.normal(0, 0.15, (nq - 100, 3)).astype(np.float32)
    q[-300:-100, :3] += rng.normal(0, 0.6, (200, 3)).astype(np.float32)
    q[-100:, :3] += 50.0
    return q


def _check_index(g, rng, what, min_accepted=(0, 0)):
    for which, m in enumerate(g.get_map_ds()):
        q = _queries(rng, m)
        want_i, want_d = _brute_knn(m, q)
        got_i, got_d = g.debug_knn(which, q)
        assert (want_i[:, 4] >= 0).sum() >= min_accepted[which], f"{what}: the case should have accepted queries"
        np.testing.assert_array_equal(got_i, want_i, err_msg=f"{what}, segment {which}: neighbours")
        np.testing.assert_array_equal(bits(got_d), bits(want_d), err_msg=f"{what}, segment {which}: squared distances")


def _box(rng, n, lo, hi):
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = rng.uniform(lo, hi, (n, 3))
    pts[:, 3] = rng.uniform(0, 200, n)
    return pts


def _blobs(rng, n, centres, sigma=0.8):
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = np.asarray(centres, np.float64)[rng.integers(0, len(centres), n)] + rng.normal(0, sigma, (n, 3)) * [1, 1, 0.3]
    pts[:, 3] = rng.uniform(0, 200, n)
    return pts


@pytest.fixture(scope="module")
def scene(pkg, oracle):
    return make_small_scene(pkg, oracle, n_raw=12001, n_kf=8)


def _case_maps(name, scene):
    """(corner raw, surf raw, accepted queries to expect per segment, check of the property the case is named for)"""
    rng = np.random.default_rng(97)
    P = SMALL["max_map_points"]
    if name == "empty_corner":
        return np.zeros((0, 4), np.float32), _box(rng, 6000, [-6, -6, -1], [6, 6, 1]), (0, 300), None
    if name == "one_point":
        return _box(rng, 1, 2, 3), _box(rng, 1, -3, -2), (0, 0), None
    if name == "one_cell":                                  # every centroid in cell (2, 2, 2) of a 6 x 6 x 6 grid
        c, s = _box(rng, 3000, 10.05, 10.45), _box(rng, 3000, 10.05, 10.45)
        return c, s, (300, 300), lambda: all((np.floor((xyzi(r)[:, :3] - 9.0) * 2.0) == 2).all() for r in (c, s))
    if name == "fewer_cells_than_chunks":                   # L = 1: a chunk is one cell
        c, s = _box(rng, 4000, [0.05, 0.05, 0.05], [1.95, 2.95, 0.95]), _box(rng, 4000, [0.05, 0.05, 0.05], [1.95, 2.95, 0.95])
        return c, s, (300, 100), lambda: all(1 < _geometry(r, P)[0].prod() < GRID_SCAN_BLOCKS for r in (c, s))
    if name == "ragged_last_chunk":
        c, s = _box(rng, 6000, [-7, -5, -1], [6, 8, 1.5]), _box(rng, 9000, [-7, -5, -1], [6, 8, 1.5])
        return c, s, (300, 300), lambda: all(_geometry(r, P)[0].prod() % GRID_SCAN_BLOCKS != 0 and _geometry(r, P)[0].prod() > 4 * GRID_SCAN_BLOCKS and _geometry(r, P)[1] == 1 for r in (c, s))
    if name == "one_metre_cells":
        centres = [[x, y, z] for x in (-28, 0, 27) for y in (-29, 1, 28) for z in (-4, 4)]
        c, s = _blobs(rng, 9000, centres), _blobs(rng, 9000, centres)
        return c, s, (300, 300), lambda: all(_geometry(r, P)[1] == 2 for r in (c, s))
    if name == "pcl_overflow":                              # surf: more than 2^31 voxels of 0.4 m → output = input
        c, s = _box(rng, 3000, [-4, -4, -1], [4, 4, 1]), _box(rng, 3000, [-4, -4, -1], [4, 4, 1])
        s[:2, :3] = [[-300, -300, -300], [300, 300, 300]]
        return c, s, (300, 300), lambda: float(np.prod(np.floor(600 / 0.4) + np.ones(3))) > 2.0 ** 31
    if name == "scene":
        return scene["map_corner"], scene["map_surf"], (300, 300), None
    raise KeyError(name)


CASES = ["empty_corner", "one_point", "one_cell", "fewer_cells_than_chunks", "ragged_last_chunk", "one_metre_cells", "pcl_overflow", "scene"]


@pytest.mark.parametrize("mode", [1, 2], ids=["sorted_standalone_count", "binned_count_in_vb_copy"])
@pytest.mark.parametrize("name", CASES)
def test_index_is_exact(pkg, hip, scene, name, mode):
    c, s, accepted, prop = _case_maps(name, scene)
    assert prop is None or prop(), f"{name}: the map does not have the property the case is named for"
    g = pkg.LidarHotpath(hip, **small_params(voxel_mode=mode, **({} if name == "scene" else SMALL)))
    g.map_set(c, s)
    n = g.counts()
    if name == "empty_corner":
        assert n["map_corner_ds"] == 0 and n["map_surf_ds"] > 500
    if name == "one_point":
        assert n["map_corner_ds"] == 1 and n["map_surf_ds"] == 1
    if name == "pcl_overflow":
        assert n["map_surf_ds"] == len(s) and n["map_corner_ds"] < len(c)
    _check_index(g, np.random.default_rng(5), f"{name}, voxel_mode {mode}", accepted)
    g.close()


@pytest.mark.parametrize("mode", [1, 2], ids=["sorted_standalone_count", "binned_count_in_vb_copy"])
def test_small_map_after_a_large_one(pkg, hip, scene, mode):
    """the chunk totals of one build must not reach the next: large, small, large again on one handle, and a rebuild of the same map"""
    rng = np.random.default_rng(7)
    large = (scene["map_corner"], scene["map_surf"])
    small = (_box(rng, 500, [20, 20, 0], [22, 22, 1]), _box(rng, 800, [20, 20, 0], [22, 22, 1]))
    g = pkg.LidarHotpath(hip, **small_params(voxel_mode=mode))
    for step, (c, s) in enumerate((large, small, large)):
        g.map_upload(c, s); g.map_build()
        _check_index(g, rng, f"voxel_mode {mode}, build {step}")
        g.map_build()
        _check_index(g, rng, f"voxel_mode {mode}, build {step} again")
    g.close()


def test_incremental_map_then_match(pkg, oracle, hip):
    """lvi_map_update (inc_out in front of the stand-alone count): exact index at every step, then a match with the bits of the
    handle that assembles and rebuilds the same keys"""
    S = pkg.synth
    KF = dict(max_keyframes=16, max_keyframe_points=200000)
    o = pkg.LidarHotpath(oracle, **small_params())
    kfs = []
    for k in range(5):
        pose = S.loop_pose(0.2 + 0.11 * k, 0.01 * np.sin(k), -0.01 * np.cos(k)).astype(np.float32)
        o.scan_upload(S.make_scan(12001, pose, 800 + k)); o.scan_organize(); o.scan_extract(); o.scan_downsample()
        c, s = o.get_scan_ds()
        kfs.append((c.copy(), s.copy(), pose))
    o.close()
    a = pkg.LidarHotpath(hip, **small_params(**KF))
    b = pkg.LidarHotpath(hip, **small_params(**KF))
    for h in (a, b):
        for c, s, pose in kfs:
            h.keyframe_add(c, s, pose)
    pose_q = S.loop_pose(0.45, 0.0, 0.01)
    scan = S.make_scan(12001, pose_q, 4242)
    guess = S.perturbed_guess(pose_q, 3)
    rng = np.random.default_rng(3)
    for keys in ([0, 1, 2, 3, 4], [2], [1, 2, 3, 3]):
        a.map_update(keys); b.map_assemble(keys)
        for x, y in zip(a.get_map_ds(), b.get_map_ds()):
            np.testing.assert_array_equal(xyzi(x).view(np.uint32), xyzi(y).view(np.uint32))
        _check_index(a, rng, f"incremental map, keys {keys}", (100, 300))
        recs = []
        for h in (a, b):
            h.scan_upload(scan); h.scan_organize(); h.scan_extract(); h.scan_downsample()
            recs.append(h.scan_match(guess))
        np.testing.assert_array_equal(bits(recs[0]["pose"]), bits(recs[1]["pose"]))
        assert recs[0]["n_sel"] == recs[1]["n_sel"] and recs[0]["status"] == recs[1]["status"] == 0
    a.close(); b.close()


# ----------------------------------------------------------------------------- batch handles
NB = 8
BATCH_P = dict(icp_max_iters=6, icp_disable_break=1, voxel_mode=2)


@pytest.fixture(scope="module")
def batch_ref(pkg, hip, scene):
    """scans, guesses and the scan_match record of every scan from a one-slot handle that rebuilds the map for each"""
    S = pkg.synth
    poses = [S.loop_pose(0.37 + 0.3 * k, 0.01 * k, -0.01) for k in range(NB)]
    scans = [S.make_scan(9001 + 700 * k, poses[k], 900 + k) for k in range(NB)]
    guesses = np.stack([S.perturbed_guess(poses[k], 20 + k) for k in range(NB)])
    g = pkg.LidarHotpath(hip, batch_scans=1, **small_params(**BATCH_P))
    g.map_upload(scene["map_corner"], scene["map_surf"]); g.map_build()
    recs = []
    for k in range(NB):
        g.batch_upload(scans[k:k + 1]); g.batch_run(guesses[k:k + 1], 0, rebuild_map=True)
        recs.append(g.batch_get_records(1)[0].view(np.uint32).copy())
    g.close()
    return scans, guesses, recs


def _launches_of(g, fn):
    g.prof_reset()
    fn()
    return {r["name"]: r["launches"] for r in g.prof_read()}


@pytest.mark.parametrize("slots", [1, 3, 8])
def test_batch_slots(pkg, hip, scene, batch_ref, slots):
    scans, guesses, ref = batch_ref
    b = pkg.LidarHotpath(hip, batch_scans=slots, **small_params(**BATCH_P))
    b.map_upload(scene["map_corner"], scene["map_surf"]); b.map_build()
    for rep in range(2):                                  # (the second run rebuilds every slot's index over the first one's)
        b.batch_upload(scans[:slots]); b.batch_run(guesses[:slots], 0, rebuild_map=True)
        recs = b.batch_get_records(slots)
        for k in range(slots):
            np.testing.assert_array_equal(recs[k].view(np.uint32), ref[k], err_msg=f"run {rep}, slot {k}")
            assert int(recs[k, 6:7].view(np.int32)[0]) == 0
    rng = np.random.default_rng(11)
    for z in range(slots):
        b.batch_select(z)
        _check_index(b, rng, f"{slots} slots, slot {z}", (300, 300))
    b.batch_select(0)
    # the launches of the index: none for the chunk totals, none for the count behind a binned rebuild
    b.prof_enable(True)
    n = _launches_of(b, b.map_build)
    assert "grid_scan_sum" not in n and "grid_count" not in n, n
    assert n.get("grid_scan_apply") == 1 and n.get("grid_scatter") == 1 and n.get("vb_copy/map") == 1, n
    b.close()


def test_launches_of_the_other_producers(pkg, hip, scene):
    """sorted realisation: the stand-alone count, still no pass for the chunk totals"""
    g = pkg.LidarHotpath(hip, **small_params(voxel_mode=1))
    g.prof_enable(True)
    g.map_upload(scene["map_corner"], scene["map_surf"])
    n = _launches_of(g, g.map_build)
    assert "grid_scan_sum" not in n and "vb_copy/map" not in n, n
    assert n.get("grid_count") == 1 and n.get("grid_scan_apply") == 1 and n.get("grid_scatter") == 1, n
    g.close()
