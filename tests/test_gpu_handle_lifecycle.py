"""The lifecycle of the ten stand-alone handles that open and close through one scaffold (csrc/lvi_dev.hpp):
fman, marg, win, pgo, kf, bow, depth, fmat, fmatb, pnp, each through its Python class and its module's small scene.

  smallest capacities   create at the smallest legal capacities, close, close again
  two handles           two handles alive on one device, fed one scene with their calls interleaved, give the bytes of each
                        other and of a third handle that ran alone: no staging is shared between handles
  create and close      30 times; the free device memory afterwards is within one arena of its value before.  Only the device
                        side is observable this way: torch.cuda.mem_get_info does not see pinned host memory, so nothing
                        here speaks about the pinned arena.
  invalid capacity      one out-of-range capacity per kind: LVI_ERR_INVALID_ARG and the text of the create function

The arena of the memory test is bounded from below: `arena` of a kind is the sum of the handle's largest device arrays
as its header and its carve state them, computed from the capacities.  The real arena is larger, so the check is
tighter than "one arena", never looser.
"""
import os

import numpy as np
import pytest

import bow_ref as B
import depth_scenes as DS
import fman_ref as FR
import fmat_ref as MR
import marg_ref as GR
import pgo_ref as PR
import pnp_ref as NR
import test_gpu_kf as TK
import test_gpu_marg as TM
import test_gpu_win as TW

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROUNDS = 30


def _bytes(*arrays):
    return [np.ascontiguousarray(a).tobytes() for a in arrays]


class Kind:
    """one handle kind: make(caps) -> handle, the scene as a list of phases (handle, state dict), the result as bytes"""
    caps = {}          # the capacities of the scene and of the memory test
    small = {}         # the smallest legal capacities
    bad = {}           # one out-of-range capacity
    bad_text = ""

    def __init__(self, pkg, hip):
        self.pkg, self.hip = pkg, hip

    def make(self, **caps):
        raise NotImplementedError

    def close(self, h):
        h.close()

    def close_twice(self, h):
        h.close()
        h.close()


class Fman(Kind):
    caps = dict(max_features=64)
    small = dict(max_features=1)
    bad = dict(max_features=0)
    bad_text = "max_features is outside 1..LVI_FMAN_MAX_FEATURES"

    def make(self, **caps):
        return self.pkg.FeatureTable(self.hip, **caps)

    def arena(self, max_features):
        return 2 * self.pkg.FeatureTable.feature_dtype.itemsize * max_features           # the two tables

    def phases(self):
        sc = FR.window_scene(77, 12)
        frames = [(ids, np.asarray(obs, np.float64).reshape(-1, 8)) for ids, obs in sc["frames"]]

        def add(h, s):
            for i, (ids, obs) in enumerate(frames):
                h.add_frame(i, ids, obs, 0.0)

        def tri(h, s):
            s["tri"] = h.triangulate(sc["Ps"], sc["Rs"], sc["tic"], sc["ric"])
        return [add, tri]

    def result(self, h, s):
        tab = h.download()
        tab["reserved"] = 0
        for f in tab:
            f["obs"][int(f["n_obs"]):] = 0                               # observations past n_obs are not defined (fman_ref.same_table)
        return _bytes(tab, h.depth_vector()) + [repr(sorted(s["tri"].items()))]


class Marg(Kind):
    caps = dict(max_blocks=512, max_projections=512, max_dense_factors=2, max_dense_rows=128, max_drop_dim=160, max_keep_dim=96)
    small = dict(max_blocks=1, max_projections=1, max_dense_factors=0, max_dense_rows=0, max_drop_dim=1, max_keep_dim=1)
    bad = dict(max_blocks=0)
    bad_text = "a capacity is outside 1..LVI_MARG_MAX_*"

    def make(self, **caps):
        return self.pkg.Marginalizer(self.hip, **caps)

    def arena(self, max_drop_dim, max_keep_dim, **_):
        P = max_drop_dim + max_keep_dim + 1
        return 8 * (P * P + 3 * max_drop_dim ** 2 + 2 * max_keep_dim ** 2)               # A; Wm, Vm, Minv; Wn, Vn

    def phases(self):
        sc = GR.gpu_scene("three_td")

        def declare(h, s):
            TM._params(h, sc)
            s["dev"] = GR.play(sc, TM.Device(h))
            s["dev"]._flush()

        def run(h, s):
            s["info"] = h.marginalize()
        return [declare, run]

    def result(self, h, s):
        J, r = h.prior()
        A, b = h.debug_system()
        return _bytes(J, r, A, b) + [repr(sorted(s["info"].items()))]


class Win(Kind):
    caps = dict(max_blocks=256, max_projections=512, max_eliminated=160, max_imu=12, max_prior_rows=128, max_dim=192)
    small = dict(max_blocks=1, max_projections=1, max_eliminated=0, max_imu=0, max_prior_rows=0, max_dim=1)
    bad = dict(max_dim=0)
    bad_text = "a capacity is outside its range 0 or 1..LVI_WIN_MAX_*"

    def make(self, **caps):
        return self.pkg.WindowSolver(self.hip, **caps)

    def arena(self, max_dim, **_):
        return 8 * 2 * (max_dim + 1) ** 2                                                 # A and S

    def phases(self):
        def declare(h, s):
            s["dev"] = TW._device(h, "two_frames")

        def run(h, s):
            s["info"] = h.solve()
        return [declare, run]

    def result(self, h, s):
        state = s["dev"].state()
        info = s["info"]
        return _bytes(*[state[b] for b in sorted(state)]) + [repr((info["status"], info["iterations"], info["termination"], info["initial_cost"], info["final_cost"]))]


class Pgo(Kind):
    caps = dict(max_poses=64, max_loops=8)
    small = dict(max_poses=1, max_loops=0)
    bad = dict(max_poses=0)
    bad_text = "max_poses must be 1..LVI_PGO_MAX_POSES"

    def make(self, **caps):
        return self.pkg.PoseGraph(self.hip, **caps)

    def arena(self, max_poses, max_loops):
        return 8 * (6 * max_poses * (6 * max_loops + 6) + 3 * 36 * max_poses)             # Bm; D, Lo, Up

    def phases(self):
        sc = PR.gpu_scene("n37")
        P0 = sc["poses"]

        def build(h, s):
            for k in range(30):
                h.add_pose(None if k == 0 else P0[k - 1], P0[k])
            h.add_loop(29, 0, PR.pose_inv(sc["gt"][29]) @ sc["gt"][0], 0.2)

        def run(h, s):
            s["info"] = h.solve()
        return [build, run]

    def result(self, h, s):
        T, p = h.poses()
        return _bytes(T, p) + [repr(sorted(s["info"].items()))]


def _pattern(pkg):
    return pkg.config.load_brief_pattern(os.path.join(HERE, "golden", "brief_pattern.yml"))


class Kf(Kind):
    caps = dict(max_width=157, max_height=93, max_keypoints=2048, max_window=150, max_keyframes=2)
    small = dict(max_width=16, max_height=16, max_keypoints=1, max_window=1, max_keyframes=1)         # LVI_KF_MIN_SIDE
    bad = dict(max_width=15)
    bad_text = "max_width / max_height must be 16..8192"

    def make(self, **caps):
        return self.pkg.KeyframeDescriber(self.hip, _pattern(self.pkg), **caps)

    def arena(self, max_width, max_height, max_keypoints, max_window, max_keyframes):
        return 2 * max_width * max_height + max_keyframes * (48 * max_keypoints + 40 * max_window)   # blur, score; the slots

    def phases(self):
        img, win = TK._image(self.pkg, 157, 93), TK._window_points(157, 93)

        def describe(h, s):
            s["info"] = h.describe(0, img, win)
        return [describe]

    def result(self, h, s):
        g = h.get(0)
        return _bytes(g["keypoints"], g["keypoints_norm"], g["kp_desc"], g["window_xy"], g["win_desc"]) + [repr(sorted(s["info"].items()))]


class Bow(Kind):
    """a database and the keyframe store it lives on, made and closed together"""
    caps = dict(max_keypoints=256, max_entries=64)
    small = dict(max_keypoints=1, max_entries=1)
    bad = dict(max_keypoints=1, max_entries=0)
    bad_text = "max_entries must be positive and max_entries * max_keypoints below 2^31"

    def make(self, max_keypoints, max_entries):
        store = self.pkg.KeyframeDescriber(self.hip, _pattern(self.pkg), max_width=16, max_height=16, max_keypoints=max_keypoints, max_window=1, max_keyframes=2)
        try:
            return store, self.pkg.BowDatabase(self.hip, store, B.kat_vocab(), max_entries=max_entries)
        except Exception:
            store.close()
            raise

    def close(self, h):
        h[1].close()
        h[0].close()

    def close_twice(self, h):
        h[1].close()
        h[1].close()
        h[0].close()
        h[0].close()

    def arena(self, max_keypoints, max_entries):
        return 12 * max_entries * max_keypoints                                           # the pool's words and values

    def phases(self):
        def desc(n, first):
            return np.array([[B.KAT_FEATURES[(first + i) % 6], 0, 0, 0] for i in range(n)], np.uint64).reshape(-1, 4)

        def add(h, s):
            store, db = h
            for k in range(3):
                store.put(0, kp_desc=desc(20 + 7 * k, k))
                db.add(0)

        def query(h, s):
            store, db = h
            store.put(1, kp_desc=desc(33, 1))
            s["query"] = db.query(1, 4, -1)
        return [add, query]

    def result(self, h, s):
        return _bytes(*s["query"], *h[1].entry(0), *h[1].entry(2))


class Depth(Kind):
    caps = dict(max_clouds=4, max_cloud_points=4096, max_features=8, lidar_skip=0)
    small = dict(max_clouds=1, max_cloud_points=1, max_features=1, lidar_skip=0)
    bad = dict(max_clouds=0)
    bad_text = "max_clouds must be 1..LVI_DEPTH_MAX_CLOUDS"

    def make(self, **caps):
        return self.pkg.DepthRegister(self.hip, **caps)

    def arena(self, max_clouds, max_cloud_points, **_):
        return 16 * (3 * max_clouds * max_cloud_points + 2 * max_cloud_points)            # ring, fused, cloud; rawIn, vOut

    def phases(self):
        cloud = DS.small()["ratio_ten"]

        def push(h, s):
            s["used"] = h.lidar_callback(cloud, DS.IDENT, 0.0)

        def depth(h, s):
            s["depth"] = h.get_depth(DS.IDENT, DS.SMALL_FEATURES)
        return [push, depth]

    def result(self, h, s):
        return _bytes(s["depth"], h.get_cloud(), h.debug_range()) + [repr(s["used"])]


def _fmat_trace(t):
    return _bytes(t["subsets"], t["nmodels"], t["F"], t["score"])


class Fmat(Kind):
    caps = dict(max_points=64, max_iters=100)
    small = dict(max_points=7, max_iters=1)
    bad = dict(max_points=6, max_iters=100)
    bad_text = "max_points must be 7..LVI_FMAT_MAX_POINTS"

    def make(self, **caps):
        return self.pkg.FundamentalRansac(self.hip, **caps)

    def arena(self, max_points, max_iters):
        return (27 * 8 + 4 * 4) * max_iters + 16 * max_points                             # F, nm, score; the points

    def phases(self):
        p1, p2, _, _ = MR.two_view(40, 0.3, 0.3, seed=1040)

        def find(h, s):
            s["find"] = h.find(p1, p2, 1.0, with_info=True)
        return [find]

    def result(self, h, s):
        st, info = s["find"]
        return _bytes(st, info["F"]) + _fmat_trace(h.trace()) + [repr((info["iters"], info["best_iter"], info["n_inliers"]))]


class Fmatb(Kind):
    caps = dict(slots=2, max_points=64, max_iters=100)
    small = dict(slots=1, max_points=7, max_iters=1)
    bad = dict(slots=0, max_points=64, max_iters=100)
    bad_text = "slots must be 1..LVI_TRACKER_MAX_BATCH"

    def make(self, **caps):
        return self.pkg.FundamentalRansacBatch(self.hip, **caps)

    def arena(self, slots, max_points, max_iters):
        return slots * ((27 * 8 + 4 * 4) * max_iters + 16 * max_points)

    def phases(self):
        pairs = [MR.two_view(40 + 9 * k, 0.3, 0.3, seed=2040 + k)[:2] for k in range(2)]

        def find(h, s):
            s["find"] = h.find(pairs, 1.0)
        return [find]

    def result(self, h, s):
        out = []
        for k, (st, info) in enumerate(s["find"]):
            out += _bytes(st, info["F"]) + _fmat_trace(h.trace(k)) + [repr((info["iters"], info["best_iter"], info["n_inliers"]))]
        return out


class Pnp(Kind):
    caps = dict(max_points=64, max_iters=100)
    small = dict(max_points=5, max_iters=1)
    bad = dict(max_points=4, max_iters=100)
    bad_text = "max_points must be 5..LVI_PNP_MAX_POINTS"

    def make(self, **caps):
        return self.pkg.PnPRansac(self.hip, **caps)

    def arena(self, max_points, max_iters):
        return (12 * 8 + 3 * 4) * max_iters + 20 * max_points                             # Rt, has, good, wb; the points

    def phases(self):
        p3, p2, _, _ = NR.scene(40, 0.3, 0.5 / NR.FOCAL_LENGTH, 77)

        def solve(h, s):
            s["solve"] = h.solve(p3, p2, with_info=True)
        return [solve]

    def result(self, h, s):
        st, info = s["solve"]
        t = h.trace()
        return _bytes(st, info["R"], info["t"], t["subsets"], t["has_model"], t["R"], t["t"], t["good"]) + [repr((info["iters"], info["best_iter"], info["n_inliers"]))]


KINDS = dict(fman=Fman, marg=Marg, win=Win, pgo=Pgo, kf=Kf, bow=Bow, depth=Depth, fmat=Fmat, fmatb=Fmatb, pnp=Pnp)


@pytest.fixture(params=list(KINDS))
def kind(request, pkg, hip):
    return KINDS[request.param](pkg, hip)


def test_smallest_capacities(kind):
    kind.close_twice(kind.make(**kind.small))


def test_two_handles_interleaved_equal_one_alone(kind):
    phases = kind.phases()
    a, b = kind.make(**kind.caps), kind.make(**kind.caps)
    try:
        sa, sb = {}, {}
        for ph in phases:
            ph(a, sa)
            ph(b, sb)
        ra, rb = kind.result(a, sa), kind.result(b, sb)
    finally:
        kind.close(b)
        kind.close(a)
    c = kind.make(**kind.caps)
    try:
        sc = {}
        for ph in phases:
            ph(c, sc)
        rc = kind.result(c, sc)
    finally:
        kind.close(c)
    assert len(ra) == len(rb) == len(rc) and sum(len(x) for x in rc) > 0
    for k, (x, y, z) in enumerate(zip(ra, rb, rc)):
        assert x == y, f"result {k}: the two interleaved handles differ"
        assert x == z, f"result {k}: an interleaved handle differs from the handle that ran alone"


def test_create_and_close_gives_the_device_memory_back(kind):
    import torch
    kind.close(kind.make(**kind.caps))                                 # the runtime's own first-use allocations are not the handle's
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(ROUNDS):
        kind.close(kind.make(**kind.caps))
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    arena = kind.arena(**kind.caps)
    print(f"free before {before}, after {after}, arena >= {arena}")
    assert arena > 0 and after >= before - arena, (before, after, arena)


def test_invalid_capacity(kind):
    caps = dict(kind.caps)
    caps.update(kind.bad)
    with pytest.raises(kind.pkg.LviError) as e:
        kind.make(**caps)
    assert e.value.code == kind.pkg._abi.LVI_ERR_INVALID_ARG
    assert f"({kind.bad_text})" in str(e.value)
