"""GPU tier (-m gpu) of the batch tracker handle (include/lvi_tbatch.h).  The yardstick of every test is S separate
TrackerHotpath handles over the HIP library, given the same calls slot by slot (tests/test_gpu_tracker.py holds those bit-exact
against the oracle): every slot of the batch must return the same bits, and a stage must cost the same launches whatever the
number of slots."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from helpers import bits

pytestmark = pytest.mark.gpu

W, H = 320, 240
COUNTS = (0, 1, 63, 64, 65, 150)                 # around the wavefront size; 150 = MAX_CNT


@pytest.fixture(scope="module")
def seqs(pkg):
    """per size, 8 slots x 4 frames: a texture of the slot's own seed and three small-motion warps of it (computed once, read only)"""
    S = pkg.synth
    out = {}
    for (w, h) in ((W, H), (163, 117)):
        per_slot = []
        for s in range(8):
            img0 = S.make_texture(w, h, 1000 + 17 * s)
            per_slot.append([img0] + [S.warp_homography(img0, S.small_motion_homography(w, h, 300 + 10 * s + r, max_px=3.0)) for r in range(3)])
        out[(w, h)] = per_slot
    return out


@pytest.fixture(scope="module")
def yaml_cam():
    ref = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_params.json")))["camera"]
    return {k: float(ref[k]) for k in ("xi", "k1", "k2", "p1", "p2", "gamma1", "gamma2", "u0", "v0")}


def _points(rng, w, h, n):
    """n points: on and beyond the border first (test_lk_border_and_degenerate_points' list), then random ones around the image"""
    special = np.array([[0.0, 0.0], [w - 1.0, h - 1.0], [-40.0, 10.0], [w + 40.0, 20.0], [3.5, h - 2.25], [w / 2, h / 2], [10.75, 10.25]], np.float32)
    rnd = np.stack([rng.uniform(-5, w + 5, n), rng.uniform(-5, h + 5, n)], axis=1).astype(np.float32)
    return np.concatenate([special, rnd])[:n].copy() if n >= len(special) else np.concatenate([special[5:], rnd])[:n].copy()


def _handles(pkg, hip, slots, **kw):
    singles = [pkg.TrackerHotpath(hip, **kw) for _ in range(slots)]
    batch = pkg.TrackerBatch(hip, slots, **kw)
    return singles, batch


def _close(singles, batch):
    for t in singles:
        t.close()
    batch.close()


def _dbg(fn, A, pkg):
    """a debug item, or the status code it is refused with (a pyramid level beyond the early return)"""
    try:
        return fn()
    except pkg.LviError as e:
        return e.code


def _same(a, b, msg):
    if isinstance(a, int) or isinstance(b, int):
        assert isinstance(a, int) and isinstance(b, int) and a == b, msg
    else:
        np.testing.assert_array_equal(a, b, err_msg=msg)


def _assert_un_equal(a, b, msg):
    assert a.shape == b.shape, msg
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=msg)
    ok = ~np.isnan(a)
    np.testing.assert_array_equal(bits(a)[ok], bits(b)[ok], err_msg=msg)


# --------------------------------------------------------------------------------------------- 1. LK
@pytest.mark.parametrize("equalize", (False, True))
@pytest.mark.parametrize("size", ((W, H), (163, 117)))
@pytest.mark.parametrize("slots", (1, 3, 8))
def test_lk_and_pyramids_equal_the_single_handles(pkg, hip, seqs, slots, size, equalize):
    """three rounds of push / set_points / run_lk / get_lk; slot 1 sits round 2 out (no push, no points) and rejoins in round 3,
    where it tracks from its round-1 image.  163 x 117: odd sizes at every level, tiles that end inside the image, and the
    pyramid's early return (level 3 is never built)."""
    A = pkg._abi
    w, h = size
    singles, batch = _handles(pkg, hip, slots, max_width=W, max_height=H, max_features=256)
    try:
        if equalize:
            batch.set_equalize(True, 3.0, (8, 8))
            for t in singles:
                t.set_equalize(True, 3.0, (8, 8))
        seq = seqs[size]
        batch.push_images([seq[s][0] for s in range(slots)])
        for s, t in enumerate(singles):
            t.push_image(seq[s][0])
        rng = np.random.default_rng(slots * 100 + w)
        for rnd in (1, 2, 3):
            out = [s == 1 and rnd == 2 for s in range(slots)]
            pts = [None if out[s] else _points(rng, w, h, COUNTS[(s + rnd) % len(COUNTS)]) for s in range(slots)]
            batch.push_images([None if out[s] else seq[s][rnd] for s in range(slots)])
            batch.set_points(pts)
            batch.run_lk()
            for s, t in enumerate(singles):
                if out[s]:
                    continue
                t.push_image(seq[s][rnd]); t.set_points(pts[s]); t.run_lk()
            for s, t in enumerate(singles):
                tag = f"slots={slots} {w}x{h} eq={equalize} round {rnd} slot {s}"
                if not out[s]:
                    xb, sb, eb = batch.get_lk(s)
                    xs, ss, es = t.get_lk()
                    assert len(xb) == len(pts[s]) == len(xs), tag
                    np.testing.assert_array_equal(sb, ss, err_msg=tag)
                    np.testing.assert_array_equal(bits(xb), bits(xs), err_msg=tag)
                    np.testing.assert_array_equal(bits(eb), bits(es), err_msg=tag)
                    if len(pts[s]) >= 63 and not equalize:
                        assert sb.sum() > 0.5 * len(sb), tag                    # the comparison is not between two failures
                for what in (A.TDBG_PYRAMID_L1, A.TDBG_PYRAMID_L2, A.TDBG_PYRAMID_L3):
                    _same(_dbg(lambda: batch.debug_get(s, what, np.uint8), A, pkg), _dbg(lambda: t.debug_get(what, np.uint8), A, pkg), f"{tag} level {what}")
        if size == (163, 117):
            assert _dbg(lambda: batch.debug_get(0, A.TDBG_PYRAMID_L3, np.uint8), A, pkg) == A.LVI_ERR_STATE       # the early return was taken
    finally:
        _close(singles, batch)


# --------------------------------------------------------------------------------------------- 2. frame end
@pytest.mark.parametrize("radius", (20, 3))
def test_frame_end_equals_the_single_handles(pkg, hip, seqs, yaml_cam, radius):
    """circles (points inside, on and beyond the border) -> GFTT with quotas {150, 1, sits out} -> finish_frame with one camera per
    slot.  Slot 2 takes no GFTT and brings no kept points: n_new = 0 and nothing undistorted."""
    A = pkg._abi
    slots = 3
    kw = dict(max_width=W, max_height=H, max_features=1024, min_dist=float(radius))
    singles, batch = _handles(pkg, hip, slots, **kw)
    try:
        rng = np.random.default_rng(5 + radius)
        edge = np.array([[0.0, 0.0], [W - 1.0, H - 1.0], [W / 2 + 0.5, H / 2 - 0.5], [19.5, 20.5], [W - 20.0, 5.49]])
        kept = [np.concatenate([np.stack([rng.uniform(-10, W + 10, 40 + 10 * s), rng.uniform(-10, H + 10, 40 + 10 * s)], axis=1), edge]).astype(np.float32) for s in range(2)]
        inside = [k[(k[:, 0] >= 0) & (k[:, 0] < W) & (k[:, 1] >= 0) & (k[:, 1] < H)] for k in kept]
        cams = [dict(yaml_cam, u0=yaml_cam["u0"] * W / 1024 + 3.0 * s, v0=yaml_cam["v0"] * H / 576 - 2.0 * s) for s in range(slots)]
        quota = [150, 1, None]
        seq = seqs[(W, H)]
        batch.push_images([seq[s][0] for s in range(slots)])
        batch.set_mask_circles([kept[0], kept[1], None], radius)
        batch.run_gftt_async(quota)
        res = batch.finish_frame([inside[0], inside[1], np.zeros((0, 2), np.float32)], cams)
        assert batch.redo_mask() == 0
        for s, t in enumerate(singles):
            tag = f"radius {radius} slot {s}"
            t.push_image(seq[s][0])
            if s < 2:
                t.set_mask_circles(kept[s], radius)
                t.run_gftt_async(quota[s])
                new, un = t.finish_frame(inside[s], cams[s])
                np.testing.assert_array_equal(batch.debug_get(s, A.TDBG_MASK, np.uint8), t.debug_get(A.TDBG_MASK, np.uint8), err_msg=tag)
                assert int(batch.debug_get(s, A.TDBG_GFTT_NCAND, np.int32)[0]) == int(t.debug_get(A.TDBG_GFTT_NCAND, np.int32)[0]), tag
            else:
                new, un = t.finish_frame(np.zeros((0, 2), np.float32), cams[s])
            nb, ub = res[s]
            np.testing.assert_array_equal(bits(nb), bits(new), err_msg=tag)
            _assert_un_equal(ub, un, tag)
        assert len(res[0][0]) > 20 and len(res[1][0]) == 1 and len(res[2][0]) == 0 and len(res[2][1]) == 0
        assert len(res[0][1]) == len(inside[0]) + len(res[0][0])
    finally:
        _close(singles, batch)


# --------------------------------------------------------------------------------------------- 3. GFTT overflow
@pytest.mark.parametrize("radix", (False, True))
def test_gftt_overflow_redoes_only_that_slot(pkg, hip, seqs, yaml_cam, monkeypatch, radix):
    """slot 1 gets the tiled 64 x 64 patch of test_mask_from_circles_sortpick_and_one_read_frame_end at max_features = 4096, quota 0
    and min_dist 3: 2296 corners pass the distance filter (CPU oracle), more than the 2048 the LDS form's accepted list holds, so
    that slot reports -2 and is redone alone in the radix form.  The others keep the results of the first read."""
    if radix:
        monkeypatch.setenv("LVI_GFTT_RADIX", "1")
    else:
        monkeypatch.delenv("LVI_GFTT_RADIX", raising=False)
    slots = 3
    kw = dict(max_width=W, max_height=H, max_features=4096, min_dist=3.0)
    singles, batch = _handles(pkg, hip, slots, **kw)
    try:
        seq = seqs[(W, H)]
        tiled = np.tile(pkg.synth.make_texture(W, H, 4242)[:64, :64], (H // 64 + 1, W // 64 + 1))[:H, :W].copy()
        imgs = [seq[0][0], tiled, seq[2][0]]
        kept = [np.array([[50.0 + 10 * s, 60.0], [200.0, 100.0 + s]], np.float32) for s in range(slots)]
        quota = [40, 0, 40]
        cams = [dict(yaml_cam, u0=0.5 * W + s, v0=0.5 * H) for s in range(slots)]
        batch.push_images(imgs)
        batch.set_mask_circles(kept, 3)
        batch.run_gftt_async(quota)
        res = batch.finish_frame(kept, cams)
        assert batch.redo_mask() == (0 if radix else 1 << 1)
        for s, t in enumerate(singles):
            t.push_image(imgs[s]); t.set_mask_circles(kept[s], 3); t.run_gftt_async(quota[s])
            new, un = t.finish_frame(kept[s], cams[s])
            np.testing.assert_array_equal(bits(res[s][0]), bits(new), err_msg=f"slot {s}")
            _assert_un_equal(res[s][1], un, f"slot {s}")
        assert len(res[1][0]) > 2048 and len(res[0][0]) == 40 and len(res[2][0]) == 40
    finally:
        _close(singles, batch)


# --------------------------------------------------------------------------------------------- 4. launch counts
def _frame(batch, seq, take, rnd, rng):
    """one full frame for the slots of `take`: push (with CLAHE), LK, circles, GFTT, frame end"""
    n = batch.slots
    batch.push_images([seq[s][rnd] if take[s] else None for s in range(n)])
    batch.set_points([_points(rng, W, H, 150) if take[s] else None for s in range(n)])
    batch.run_lk()
    kept = []
    for s in range(n):
        if not take[s]:
            kept.append(None)
            continue
        xy, st, _ = batch.get_lk(s)
        k = xy[st == 1]
        kept.append(k[(k[:, 0] >= 0) & (k[:, 0] < W) & (k[:, 1] >= 0) & (k[:, 1] < H)])
    batch.set_mask_circles(kept, 20)
    batch.run_gftt_async([max(150 - len(kept[s]), 1) if take[s] else None for s in range(n)])
    cam = dict(xi=1.4, k1=-0.03, k2=0.26, p1=0.001, p2=0.0003, gamma1=1454.0, gamma2=1451.0, u0=0.5 * W, v0=0.5 * H)
    batch.finish_frame(kept, [cam if take[s] else None for s in range(n)])
    assert batch.redo_mask() == 0


def test_launch_counts_do_not_depend_on_the_slots(pkg, hip, seqs):
    """every kernel's launches for one full frame (no redo): the same for 1, 3 and 8 slots, and with 3 of 8 slots taking part"""
    seq = seqs[(W, H)]
    counts = {}
    for name, slots, take in (("1", 1, [True]), ("3", 3, [True] * 3), ("8", 8, [True] * 8), ("3 of 8", 8, [True, False, True, False, False, True, False, False])):
        b = pkg.TrackerBatch(hip, slots, max_width=W, max_height=H, max_features=256)
        try:
            b.set_equalize(True, 3.0, (8, 8))
            rng = np.random.default_rng(3)
            b.push_images([seq[s][0] for s in range(slots)])          # every slot has its pair before the counted frame
            _frame(b, seq, [True] * slots, 1, rng)
            b.prof_enable(True); b.prof_reset()
            _frame(b, seq, take, 2, rng)
            counts[name] = {r["name"]: r["launches"] for r in b.prof_read()}
            b.prof_enable(False)
        finally:
            b.close()
    print("launches per frame:", counts["8"])
    want = {"clahe_lut": 1, "clahe_interp": 1, "pyrdown": 3, "lk_track": 1, "mask_fill": 1, "mask_circles": 1, "gftt_mineig": 1, "gftt_count": 1,
            "gftt_emit": 1, "gftt_sortpick": 1, "frame_concat": 1, "mei_undistort": 1}
    for name, c in counts.items():
        assert c == want, (name, c)


# --------------------------------------------------------------------------------------------- 5. errors
def test_errors_are_atomic_and_follow_the_single_handle(pkg, hip, seqs):
    A = pkg._abi
    slots = 3
    singles, batch = _handles(pkg, hip, slots, max_width=W, max_height=H, max_features=64)
    try:
        seq = seqs[(W, H)]
        dll = hip.dll
        n = C.c_int32(0)
        buf = np.zeros((64, 2), np.float32); st = np.zeros(64, np.uint8); er = np.zeros(64, np.float32)

        def raw_get(slot):
            return dll.lvi_tbatch_get_lk(batch._b, slot, A._ptr(buf), A._ptr(st), A._ptr(er), 64, C.byref(n))

        # state errors as the single handle's: LK without an image pair, get_lk before run_lk
        rng = np.random.default_rng(9)
        good = [_points(rng, W, H, 40) for _ in range(slots)]
        batch.set_points(good)
        assert dll.lvi_tbatch_run_lk(batch._b) == A.LVI_ERR_STATE
        batch.push_images([seq[s][0] for s in range(slots)])
        batch.push_images([seq[s][1] for s in range(slots)])
        batch.set_points(good)
        assert raw_get(0) == A.LVI_ERR_STATE
        # a slot out of range
        assert raw_get(-1) == A.LVI_ERR_INVALID_ARG and raw_get(slots) == A.LVI_ERR_INVALID_ARG
        assert dll.lvi_tbatch_debug_get(batch._b, slots, A.TDBG_PYRAMID_L1, None, 0, None) == A.LVI_ERR_INVALID_ARG
        # n > max_features in slot 2: LVI_ERR_CAPACITY and no slot changes — slots 0 and 1 still run the points set before
        too_many = np.zeros((65, 2), np.float32)
        other = [_points(rng, W, H, 20) for _ in range(2)]
        with pytest.raises(A.LviError) as e:
            batch.set_points([other[0], other[1], too_many])
        assert e.value.code == A.LVI_ERR_CAPACITY
        batch.run_lk()
        for s, t in enumerate(singles):
            t.push_image(seq[s][0]); t.push_image(seq[s][1]); t.set_points(good[s]); t.run_lk()
            xs, ss, es = t.get_lk()
            xb, sb, eb = batch.get_lk(s)
            np.testing.assert_array_equal(sb, ss)
            np.testing.assert_array_equal(bits(xb), bits(xs))
            np.testing.assert_array_equal(bits(eb), bits(es))
        # bad tables are refused before anything runs
        ptrs = (C.c_void_p * slots)()
        assert dll.lvi_tbatch_push_images(batch._b, ptrs, W, H, W - 1) == A.LVI_ERR_INVALID_ARG
        assert dll.lvi_tbatch_push_images(batch._b, None, W, H, W) == A.LVI_ERR_INVALID_ARG
        assert dll.lvi_tbatch_push_images(batch._b, ptrs, W + 1, H, W + 1) == A.LVI_ERR_CAPACITY
    finally:
        _close(singles, batch)


# --------------------------------------------------------------------------------------------- 6. rig
def _rig_sequence(pkg, seed, n, cut):
    """n frames at 320 x 240: slow drift (<= 1.8 px per frame at the corners), a new texture at frame `cut`"""
    S = pkg.synth
    tex, Hacc, frames = S.make_texture(W, H, seed), np.eye(3), []
    corners = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], np.float64)
    for k in range(n):
        if k == cut:
            tex, Hacc = S.make_texture(W, H, seed + 1), np.eye(3)
        elif k > 0:
            Hm = S.small_motion_homography(W, H, seed * 1000 + k, max_px=2.0)
            d = np.abs(S.apply_homography(Hm, corners) - corners).max()
            Hacc = (np.eye(3) + min(1.0, 1.8 / max(d, 1e-12)) * (Hm - np.eye(3))) @ Hacc
        frames.append(S.warp_homography(tex, Hacc))
    return frames


def test_rig_equals_three_feature_trackers(pkg, hip, yaml_cam):
    """FeatureTrackerRig (3 cameras over one lvi_tbatch) against three FeatureTrackers over three lvi_tracker handles, both through
    the HIP host library with the same updateID loop: 40 frames, a scene cut per camera, a different PUB_THIS_FRAME pattern per
    camera, equalize on, a camera model and the device rejectWithF per camera.  cur_pts, ids, track_cnt, cur_un_pts and
    pts_velocity are bit-equal per frame and camera."""
    hl = pkg.load_host()
    slots, n = 3, 40
    seqs3 = [_rig_sequence(pkg, 70 + 5 * s, n, cut) for s, cut in zip(range(slots), (13, 22, 31))]
    pub = [lambda k: True, lambda k: k % 2 == 0, lambda k: k % 3 != 1]
    cams = [dict(yaml_cam, u0=yaml_cam["u0"] * W / 1024 + 2.0 * s, v0=yaml_cam["v0"] * H / 576 - 1.5 * s) for s in range(slots)]
    tp = pkg.default_tracker_params(hip, max_width=W, max_height=H, max_features=256, max_cnt=100, min_dist=15.0)
    runs = []
    for batched in (True, False):
        rig = pkg.host_api.TrackerRig(hl, tp, slots, H, W, equalize=True, cams=cams, batched=batched)
        try:
            rig.use_device_fundamental()
            rig.reset_ids()
            per_frame = []
            for k in range(n):
                rig.read_images([seqs3[s][k] for s in range(slots)], [100.0 + k / 30.0 + 0.001 * s for s in range(slots)], [pub[s](k) for s in range(slots)])
                rig.update_ids()
                per_frame.append([rig.camera(s) for s in range(slots)])
            runs.append(per_frame)
        finally:
            rig.close()
    longest = 0
    for k in range(n):
        for s in range(slots):
            a, b = runs[0][k][s], runs[1][k][s]
            tag = f"frame {k} camera {s}"
            np.testing.assert_array_equal(a["ids"], b["ids"], err_msg=tag)
            np.testing.assert_array_equal(a["track_cnt"], b["track_cnt"], err_msg=tag)
            np.testing.assert_array_equal(bits(a["cur_pts"]), bits(b["cur_pts"]), err_msg=tag)
            _assert_un_equal(a["cur_un_pts"], b["cur_un_pts"], tag)
            _assert_un_equal(a["pts_velocity"], b["pts_velocity"], tag)
            longest = max(longest, int(a["track_cnt"].max()) if len(a["track_cnt"]) else 0)
    # the sequences do what they are for: tracks live across many frames, every camera fills up, ids are shared out among the cameras
    assert longest >= 10
    last = runs[0][n - 1]
    assert all(len(c["ids"]) > 50 for c in last)
    allids = np.concatenate([c["ids"] for c in last])
    assert len(set(allids.tolist())) == len(allids) and (allids >= 0).all()
