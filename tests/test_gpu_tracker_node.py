"""GPU tier: the feature_tracker node (host/lvi_host.hpp FeatureTrackerNode / FeatureTracker, feature_tracker_node.cpp:37-231)
over liblvi_hip.so against the same node code over the CPU oracle, frame by frame and bit for bit.  Over the HIP library the node
takes a path of its own: the mask rastered from circles, GFTT enqueued and fetched by one lvi_tracker_finish_frame read (with the
LDS sort + pick redone in the radix form when its tables overflow), the undistorted points of that read reused by
undistortedPoints(), and LK reading its points in place from pinned slots.  Every stage is bit-exact on its own; this checks that
the composition is too: outcome, frequency control, the track set (u, v, id, track_cnt) and the published message (ids, u, v,
velocities, un_x / un_y)."""
import json
import os

import numpy as np
import pytest

from helpers import bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hostlibs(pkg, oracle, hip, tmp_path_factory):
    H = pkg.host_api
    out = tmp_path_factory.mktemp("hostlib") / "liblvi_host_oracle.so"
    H.build_host_library(str(out), os.path.dirname(oracle.path), "lvi_oracle", extra=("-fopenmp",))
    return H.HostLibrary(str(out)), pkg.load_host()


def _camera(w, h):
    """the yaml camera (params_camera.yaml through tests/golden/reference_params.json, 1024 x 576); other sizes move the
    principal point with the image"""
    c = json.load(open(os.path.join(HERE, "golden", "reference_params.json")))["camera"]
    cam = {k: float(c[k]) for k in ("xi", "k1", "k2", "p1", "p2", "gamma1", "gamma2", "u0", "v0")}
    if (w, h) != (1024, 576):
        cam["u0"], cam["v0"] = cam["u0"] * w / 1024.0, cam["v0"] * h / 576.0
    return cam


def _translation(dx, dy):
    return np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])


def _slow_step(pkg, w, h, seed, max_disp=1.8):
    """a small_motion_homography scaled towards the identity until no image corner moves more than max_disp px"""
    S = pkg.synth
    Hm = S.small_motion_homography(w, h, seed, max_px=2.0)
    c = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float64)
    d = np.abs(S.apply_homography(Hm, c) - c).max()
    a = min(1.0, max_disp / max(d, 1e-12))
    return np.eye(3) + a * (Hm - np.eye(3))


def _sequence(pkg, w, h, n, seed):
    """n frames and stamps (30 Hz): slow drift (<= 2 px per frame) so tracks live long, two pairs of 20 px jumps (there and back),
    a scene cut (a new texture), one almost uniform frame, a stamp gap > 1 s and a stamp that goes back.  Returns (frames, stamps,
    events) with events[name] = frame index."""
    S = pkg.synth
    ev = dict(fast_a=int(n * 0.30), fast_b=int(n * 0.52), gap=int(n * 0.42), cut=int(n * 0.66), flat=int(n * 0.78), back=int(n * 0.90))
    jumps = {ev["fast_a"]: (18.0, -9.0), ev["fast_a"] + 1: (-18.0, 9.0), ev["fast_b"]: (-12.0, -16.0), ev["fast_b"] + 1: (12.0, 16.0)}
    tex, Hacc = S.make_texture(w, h, seed), np.eye(3)
    frames, stamps, t = [], [], 1000.0
    for k in range(n):
        if k == ev["cut"]:
            tex, Hacc = S.make_texture(w, h, seed + 1), np.eye(3)
        elif k in jumps:
            Hacc = _translation(*jumps[k]) @ Hacc
        elif k > 0:
            Hacc = _slow_step(pkg, w, h, seed * 1000 + k) @ Hacc
        if k == ev["flat"]:
            img = np.full((h, w), 128, np.uint8)
            img[h // 2:h // 2 + 6, w // 2:w // 2 + 6] = 140            # a few corners at most
        else:
            img = S.warp_homography(tex, Hacc)
        if k == ev["gap"]:
            t += 1.5
        elif k == ev["back"]:
            t -= 0.05
        elif k > 0:
            t += 1.0 / 30.0
        frames.append(img); stamps.append(t)
    return frames, stamps, ev


class MedianFlowReject:
    """a pure rejectWithF: float64 flow of every track against the median flow; a track departing from it by more than
    `bound` * F_THRESHOLD px is rejected.  Records what it was given."""

    def __init__(self, bound):
        self.bound, self.calls, self.rejected = bound, [], 0

    def __call__(self, un_cur, un_forw, thr):
        self.calls.append((un_cur.copy(), un_forw.copy(), thr))
        f = un_forw.astype(np.float64) - un_cur.astype(np.float64)
        dev = np.hypot(*(f - np.median(f, axis=0)).T)
        st = (dev <= self.bound * thr).astype(np.uint8)
        self.rejected += int((st == 0).sum())
        return st


# name, (w, h), frames, FREQ, equalize, hook bound (None = no hook), max_cnt, min_dist, max_features, LVI_GFTT_RADIX
CONFIGS = [
    ("yaml_1024x576", (1024, 576), 90, 20, True, 1.5, 150, 20.0, 1024, False),
    ("hd_1280x720_every_frame", (1280, 720), 80, 40, False, None, 150, 20.0, 1024, False),
    ("odd_333x251_full_radix", (333, 251), 90, 20, True, 1.0, 40, 25.0, 1024, True),
    ("odd_752x480_lds_redo", (752, 480), 80, 20, False, 2.0, 2500, 5.0, 4096, False),
]
THROTTLED = {c[0] for c in CONFIGS if c[3] < 30}           # 30 Hz stamps


def _run_pair(pkg, oracle, hostlibs, monkeypatch, cfg):
    name, (w, h), n, freq, equalize, bound, max_cnt, min_dist, max_feat, radix = cfg
    H = pkg.host_api
    h_ora, h_hip = hostlibs
    tp = pkg.default_tracker_params(oracle, max_width=w, max_height=h, max_cnt=max_cnt, min_dist=min_dist, max_features=max_feat)
    cam = _camera(w, h)
    if radix:
        monkeypatch.setenv("LVI_GFTT_RADIX", "1")                     # read by lvi_tracker_create
    else:
        monkeypatch.delenv("LVI_GFTT_RADIX", raising=False)
    nodes = [H.TrackerNode(hl, tp, h, w, freq, equalize=equalize, cam=cam) for hl in (h_ora, h_hip)]
    monkeypatch.delenv("LVI_GFTT_RADIX", raising=False)
    hooks = [MedianFlowReject(bound), MedianFlowReject(bound)] if bound is not None else None
    if hooks:
        for nd, hk in zip(nodes, hooks):
            nd.set_fundamental_hook(hk)
    return nodes, hooks


def _drive(node, frames, stamps):
    return [(node.image(img, t), node.points()) for img, t in zip(frames, stamps)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_tracker_node_hip_equals_oracle(pkg, oracle, hip, hostlibs, monkeypatch, cfg):
    """two TrackerNodes, one over each library, fed the same frames and stamps: every frame's outcome, frequency decision,
    pub_count, rejectWithF count and track set, and every published message, are identical bit for bit"""
    name, (w, h), n, freq, equalize, bound, max_cnt, min_dist, max_feat, radix = cfg
    frames, stamps, ev = _sequence(pkg, w, h, n, seed=31 + len(name))
    nodes, hooks = _run_pair(pkg, oracle, hostlibs, monkeypatch, cfg)
    try:
        # one node after the other: feature ids come from FeatureTracker::n_id, a function-local static that both host libraries
        # share (a unique symbol), so each run's ids are consecutive from its first one and are compared from there
        runs = [_drive(nd, frames, stamps) for nd in nodes]
    finally:
        for nd in nodes:
            nd.close()
    outcomes, sizes, max_track, lost_half, full_no_new = [], [], 0, 0, 0
    prev_ids, id_base = None, None
    for k, ((ro, po), (rg, pg)) in enumerate(zip(*runs)):
        where = f"{name} frame {k}"
        for key in ("outcome", "pub_this_frame", "pub_count", "rejectWithF_skipped", "n_cur_pts"):
            assert ro[key] == rg[key], (where, key, ro[key], rg[key])
        assert po.shape == pg.shape, (where, po.shape, pg.shape)
        np.testing.assert_array_equal(bits(po[:, :2]), bits(pg[:, :2]), err_msg=where)
        np.testing.assert_array_equal(po[:, 3], pg[:, 3], err_msg=where)
        if id_base is None and len(po):
            id_base = (po[:, 2].min(), pg[:, 2].min())
        if id_base is not None:
            np.testing.assert_array_equal(po[:, 2] - id_base[0], pg[:, 2] - id_base[1], err_msg=where)
        if ro["outcome"] in ("published", "first_publish_suppressed"):
            cho, chg = ro["channels"], rg["channels"]
            assert cho.shape == chg.shape, where
            np.testing.assert_array_equal(cho[0] - id_base[0], chg[0] - id_base[1], err_msg=where)
            np.testing.assert_array_equal(bits(cho[1:5]), bits(chg[1:5]), err_msg=where)
            assert (cho[5] == -1.0).all() and (chg[5] == -1.0).all(), where
            Po, Pg = ro["points"], rg["points"]
            np.testing.assert_array_equal(np.isnan(Po), np.isnan(Pg), err_msg=where)
            ok = ~np.isnan(Po)
            np.testing.assert_array_equal(bits(Po)[ok], bits(Pg)[ok], err_msg=where)
            assert (Po[:, 2] == 1.0).all(), where
            assert len(Po) == int((po[:, 3] > 1).sum()), where           # only features seen in more than one frame
        # positive controls (the two sides are equal by now)
        outcomes.append(rg["outcome"]); sizes.append(len(pg))
        if len(pg):
            max_track = max(max_track, int(pg[:, 3].max()))
        ids = set(pg[:, 2].astype(np.int64).tolist())
        if prev_ids and len(prev_ids) >= 10 and len(prev_ids - ids) > len(prev_ids) / 2:
            lost_half += 1
        if rg["pub_this_frame"] and len(pg) == max_cnt and (pg[:, 3] > 1).all():
            full_no_new += 1                                              # n_max_cnt <= 0: goodFeaturesToTrack was not asked
        prev_ids = ids
    if hooks:
        ho, hg = hooks
        assert len(ho.calls) == len(hg.calls) > 10, (len(ho.calls), len(hg.calls))
        for j, (a, b) in enumerate(zip(ho.calls, hg.calls)):
            assert a[2] == b[2] == 1.0
            for x, y in zip(a[:2], b[:2]):
                assert x.shape == y.shape, (name, j)
                np.testing.assert_array_equal(bits(x), bits(y), err_msg=f"{name} hook call {j}")
        assert ho.rejected == hg.rejected > 0, (ho.rejected, hg.rejected)
    n_pub = outcomes.count("published")
    rep = dict(published=n_pub, max_track_cnt=max_track, largest_set=max(sizes), frames_losing_half=lost_half, full_no_new=full_no_new,
               rejected=hooks[1].rejected if hooks else None)
    print(name, rep)
    # the run reached what it was built to reach
    assert outcomes.count("restart") == 2 and outcomes.count("first_image") == 3, outcomes
    assert outcomes[ev["gap"]] == "restart" and outcomes[ev["back"]] == "restart"
    assert outcomes.count("first_publish_suppressed") == 1                    # init_pub is set once per node (feature_tracker_node.cpp:225-231)
    if name in THROTTLED:
        assert n_pub >= 30 and outcomes.count("not_published") >= 15, rep
    else:
        assert outcomes.count("not_published") == 0, rep
    assert max(sizes) == max_cnt, rep
    assert max_track >= 20, rep
    assert lost_half >= 1, rep
    assert full_no_new >= 1 or max_cnt > 1000, rep


def _first_frame_lds_overflows(pkg, hip, cfg):
    """the redo configuration really redoes: its first frame (an empty mask, quota max_cnt) overflows the LDS pick and
    finish_frame runs the radix form after it"""
    name, (w, h), n, freq, equalize, bound, max_cnt, min_dist, max_feat, radix = cfg
    img0 = pkg.synth.warp_homography(pkg.synth.make_texture(w, h, 31 + len(name)), np.eye(3))     # frame 0 of _sequence
    t = pkg.TrackerHotpath(hip, max_width=w, max_height=h, max_cnt=max_cnt, min_dist=min_dist, max_features=max_feat)
    t.push_image(img0)
    t.prof_enable(True); t.prof_reset()
    t.set_mask_circles(np.zeros((0, 2), np.float32), int(min_dist))
    t.run_gftt_async(max_cnt)
    new, _ = t.finish_frame(np.zeros((0, 2), np.float32), _camera(w, h))
    launches = {s["name"]: s["launches"] for s in t.prof_read()}
    t.close()
    return launches, len(new)


def test_redo_configuration_reaches_the_radix_redo(pkg, hip, monkeypatch):
    monkeypatch.delenv("LVI_GFTT_RADIX", raising=False)
    cfg = next(c for c in CONFIGS if c[0] == "odd_752x480_lds_redo")
    launches, n_new = _first_frame_lds_overflows(pkg, hip, cfg)
    print("redo configuration, first frame:", launches, "corners", n_new)
    assert launches.get("gftt_sortpick", 0) == 1 and launches.get("gftt_pick", 0) == 1, launches
    assert n_new == cfg[6] > 2048
    # and the yaml configuration does not
    launches, n_new = _first_frame_lds_overflows(pkg, hip, CONFIGS[0])
    assert launches.get("gftt_sortpick", 0) == 1 and launches.get("gftt_pick", 0) == 0, launches
    assert n_new == CONFIGS[0][6]


# ------------------------------------------------------------------------------------------------ the C-ABI call contract
@pytest.mark.parametrize("between", ["two_finish_frames", "finish_frame_with_radix_redo"])
def test_run_lk_tracks_the_points_of_the_last_set_points(pkg, oracle, hip, between):
    """lvi_tracker_run_lk tracks what the last lvi_tracker_set_points gave it, whatever lvi_tracker_finish_frame calls came
    between (oracle/lvo_tracker.cpp keeps cur_xy until the next set_points).  Other points staged by two finish_frame calls, or by
    one finish_frame that redoes the LDS pick in the radix form, leave a second LK equal to the first, bit for bit, on both sides."""
    cfg = next(c for c in CONFIGS if c[0] == "odd_752x480_lds_redo")
    name, (w, h), n, freq, equalize, bound, max_cnt, min_dist, max_feat, radix = cfg
    S = pkg.synth
    img0 = S.make_texture(w, h, 4242)
    img1 = S.warp_homography(img0, S.small_motion_homography(w, h, 7, max_px=3.0))
    cam = _camera(w, h)
    res = {}
    for lib_name, lib in (("oracle", oracle), ("hip", hip)):
        t = pkg.TrackerHotpath(lib, max_width=w, max_height=h, max_cnt=max_cnt, min_dist=min_dist, max_features=max_feat)
        P = t.good_features(img0, 120, 0.01, 20.0)
        K1 = t.good_features(img1, 300, 0.01, 9.0)[::-1].copy()             # other points, another count
        assert len(P) == 120 and len(K1) == 300
        assert not np.array_equal(P, K1[:len(P)])
        t.push_image(img0); t.push_image(img1)
        t.set_points(P); t.run_lk()
        A = t.get_lk()
        new, launches = None, None
        if between == "two_finish_frames":
            t.finish_frame(K1, cam); t.finish_frame(K1, cam)
        else:
            if lib is hip:
                t.prof_enable(True); t.prof_reset()
            t.set_mask_circles(np.zeros((0, 2), np.float32), int(min_dist))
            t.run_gftt_async(max_cnt - len(K1))                              # > 2048 accepted corners: the LDS pick overflows
            new, _ = t.finish_frame(K1, cam)
            if lib is hip:
                launches = {s["name"]: s["launches"] for s in t.prof_read()}
                t.prof_enable(False)
        t.run_lk()
        B = t.get_lk()
        res[lib_name] = (A, B, new, launches)
        t.close()
    for lib_name in ("oracle", "hip"):
        A, B, _, _ = res[lib_name]
        assert len(A[0]) == 120 and A[1].sum() > 100
        np.testing.assert_array_equal(A[1], B[1], err_msg=f"{lib_name}: status after {between}")
        np.testing.assert_array_equal(bits(A[0]), bits(B[0]), err_msg=f"{lib_name}: positions after {between}")
        np.testing.assert_array_equal(bits(A[2]), bits(B[2]), err_msg=f"{lib_name}: err after {between}")
    Ao, Ag = res["oracle"][0], res["hip"][0]
    np.testing.assert_array_equal(Ao[1], Ag[1])
    np.testing.assert_array_equal(bits(Ao[0][Ao[1] == 1]), bits(Ag[0][Ag[1] == 1]))
    if between == "finish_frame_with_radix_redo":
        np.testing.assert_array_equal(res["oracle"][2], res["hip"][2])
        assert len(res["hip"][2]) == max_cnt - 300
        launches = res["hip"][3]
        assert launches.get("gftt_pick", 0) == 1 and launches.get("gftt_sortpick", 0) == 1, launches
