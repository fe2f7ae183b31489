"""CPU tier: the hand-built depth scenes (tests/depth_scenes.py) are what they claim to be.  Conditions on the inputs of
tests/test_gpu_depth_edges.py, checked with the numpy restatement (tests/depth_ref.py) and the oracle's kd-tree only."""
import numpy as np
import pytest

import depth_ref as R
import depth_scenes as S


def _run(oracle, body_cloud, pose, feats):
    world = R.transform(R.get_transformation(oracle, pose), body_cloud)
    d, dbg = R.get_depth(oracle, world, pose, feats)
    return d, dbg


def _brute_equals_kdtree(dbg):
    if "nbr" not in dbg:
        return True
    n, s = R.brute_knn3(dbg["sphere"], dbg["V"])
    return np.array_equal(n, dbg["nbr"]) and np.array_equal(s.view(np.uint32), dbg["sqd"].view(np.uint32))


@pytest.fixture(scope="module")
def branch_runs(oracle):
    cloud, feats, labels, own = S.branches()
    return cloud, feats, labels, own, {pose: _run(oracle, cloud, pose, feats) for pose in (S.IDENT, S.POSE2)}


def test_branches_holds_every_class_at_both_poses(branch_runs):
    cloud, feats, labels, own, runs = branch_runs
    assert len(cloud) == 480 and len(feats) == 150 and all(labels.count(c) == 15 for c in S.CLASSES)
    for pose, (d, dbg) in runs.items():
        counts, taken = S.class_counts(labels, own, dbg["sphere_idx"], dbg["sphere"], dbg["nbr"], dbg["sqd"], dbg["V"], d)
        print(pose, counts, sorted(set(t for t, c in zip(taken, labels) if c == "collinear")))
        assert all(counts[c] >= 10 for c in S.CLASSES), (pose, counts)
        # the 15 duplicated points share a bin with their first copy: 465 of the 480 points reach the sphere
        assert len(dbg["sphere"]) == 465
        assert S.boundary_margin(dbg["local"]) > 0.05
        assert _brute_equals_kdtree(dbg)


def test_ties_hold_bit_equal_distances_and_a_contested_bin(oracle):
    clouds = S.ties()
    runs = {name: _run(oracle, c, S.IDENT, S.AXIS_FEATURE) for name, c in clouds.items()}
    for name, (d, dbg) in runs.items():
        assert S.boundary_margin(dbg["local"]) > 0.05 and _brute_equals_kdtree(dbg), name
        assert np.array_equal(dbg["local"].view(np.uint32), clouds[name].view(np.uint32)), name    # the identity pose moves nothing
    bits = lambda name: runs[name][1]["sqd"][0].view(np.uint32)  # noqa: E731
    nbr = lambda name: runs[name][1]["nbr"][0]  # noqa: E731
    assert bits("pairs")[0] == bits("pairs")[1] and nbr("pairs")[0] + 1 == nbr("pairs")[1]          # lower sphere index first
    assert bits("single_then_pair")[1] == bits("single_then_pair")[2] and nbr("single_then_pair")[1] + 1 == nbr("single_then_pair")[2]
    # the third place of `pairs` is contested as well: the mirror image of the third neighbour is as far and is left out
    dbg = runs["pairs"][1]
    v, sph = dbg["V"][0], dbg["sphere"]
    dx, dy, dz = (v[k] - sph[:, k] for k in range(3))
    dist = ((dx * dx + dy * dy) + dz * dz).view(np.uint32)
    assert (dist == bits("pairs")[2]).sum() == 2 and nbr("pairs")[2] == np.nonzero(dist == bits("pairs")[2])[0].min()
    # `repeated`: two cloud indices, one bin, bit-equal distance; the lower index is kept
    local = runs["repeated"][1]["local"]
    rr, cc = R.bin_angles(local)
    same_bin = (R.roundf(rr)[0] == R.roundf(rr)[3]) and (R.roundf(cc)[0] == R.roundf(cc)[3])
    assert same_bin and R.point_distance(local)[0].view(np.uint32) == R.point_distance(local)[3].view(np.uint32)
    sel = runs["repeated"][1]["sel"]
    assert (sel == 0).sum() == 1 and (sel == 3).sum() == 0
    assert np.array_equal(runs["repeated"][1]["sphere"].view(np.uint32), runs["pairs"][1]["sphere"].view(np.uint32))


def test_small_scenes_sit_on_either_side_of_the_ten_point_rule(oracle):
    for name, cloud in S.small().items():
        d, dbg = _run(oracle, cloud, S.IDENT, S.SMALL_FEATURES)
        nsph, searched = S.SMALL_EXPECT[name]
        assert len(dbg["sphere"]) == nsph and ("nbr" in dbg) == searched, name
        assert S.boundary_margin(dbg["local"]) > 0.05 and _brute_equals_kdtree(dbg), name
        if not searched:
            assert (d == -1).all(), name
    d, dbg = _run(oracle, S.small()["origin_plus_10"], S.IDENT, S.SMALL_FEATURES)
    nan = np.nonzero(np.isnan(dbg["sphere"][:, 0]))[0]
    assert len(nan) == 1 and not np.isin(dbg["nbr"], nan).any() and (dbg["nbr"] >= 0).all()
    d, dbg = _run(oracle, S.small()["origin_plus_9"], S.IDENT, S.SMALL_FEATURES)
    assert np.isnan(dbg["sphere"][:, 0]).sum() == 1 and (dbg["nbr"] >= 0).all()          # nine points still give three neighbours
    # ratio_ten: the four points at a ratio of exactly 10 are in the image, the four just above are not
    sel = _run(oracle, S.small()["ratio_ten"], S.IDENT, S.SMALL_FEATURES)[1]["sel"]
    assert set(sel[sel >= 0]) == set(range(14))
    sel = _run(oracle, S.small()["x_zero"], S.IDENT, S.SMALL_FEATURES)[1]["sel"]
    assert set(sel[sel >= 0]) == set(range(10))


def test_feature_scene_clips_its_bands_and_accepts_at_the_poles(oracle):
    cloud, f = S.features()
    d, dbg = _run(oracle, cloud, S.IDENT, f)
    assert S.boundary_margin(dbg["local"]) > 0.05 and _brute_equals_kdtree(dbg)
    assert len(dbg["sphere"]) == len(cloud)
    lo_hi = [S.band_rows(x) for x in f]
    assert lo_hi[1][0] < 0 and lo_hi[2][1] > 359 and lo_hi[3][0] <= 0 and lo_hi[4][1] >= 359
    acc = R.accepted(dbg["nbr"], dbg["sqd"])
    assert acc.tolist() == [False, False, False, True, True, True, False]
    assert (d[acc] > 3).all()
    assert np.array_equal(dbg["V"][0], np.zeros(3, np.float32))


def test_window_sequence_counts(pkg, oracle):
    W = R.Window(pkg, oracle, lidar_skip=0, window_s=1.0)
    sizes = []
    for k, cloud in enumerate(S.window_sequence()):
        ds = W.voxel(cloud)
        assert len(ds) == len(cloud), k                                        # one point per voxel
        assert int(R.fov_keep(ds).sum()) == S.WINDOW_KEPT[k], k
        assert W.lidar_callback(cloud, S.window_pose(k), S.window_stamp(k))
        sizes.append([len(c) for c in W.clouds])
    assert sizes[0] == [0] and sizes[1] == [0, 1] and sizes[6] == [513, 1025, 0] and sizes[7] == [1025, 0, 0] and sizes[8] == [0, 0, 4]
    assert all(len(s) <= 3 for s in sizes) and len(W.depth_cloud) == 4
