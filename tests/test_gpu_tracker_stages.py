"""GPU tier (-m gpu): a single tracker handle is a one-slot batch.  lvi_tracker_* and lvi_tbatch_* run the same stage
routines and the same kernels; these tests pin what the two sets of entry points promise about re-runs, empty point lists and
launches, on a single handle and on a batch alike.  163 x 117: odd at every level, partial tiles, the pyramid's early return."""
import numpy as np
import pytest

from helpers import bits

pytestmark = pytest.mark.gpu

W, H = 163, 117
KW = dict(max_width=W, max_height=H, max_features=256)
CAM = dict(xi=1.4, k1=-0.03, k2=0.26, p1=0.001, p2=0.0003, gamma1=1454.0, gamma2=1451.0, u0=0.5 * W, v0=0.5 * H)


@pytest.fixture(scope="module")
def frames(pkg):
    """a texture and two small-motion warps of it (computed once, read only)"""
    S = pkg.synth
    img0 = S.make_texture(W, H, 1000)
    return [img0] + [S.warp_homography(img0, S.small_motion_homography(W, H, 300 + r, max_px=3.0)) for r in range(2)]


@pytest.fixture(scope="module")
def points():
    rng = np.random.default_rng(11)
    return np.stack([rng.uniform(-5, W + 5, 65), rng.uniform(-5, H + 5, 65)], axis=1).astype(np.float32)


def _launches(h):
    return {r["name"]: r["launches"] for r in h.prof_read()}


def _assert_lk_equal(a, b, msg):
    assert len(a[0]) == len(b[0]), msg
    np.testing.assert_array_equal(a[1], b[1], err_msg=msg)
    np.testing.assert_array_equal(bits(a[0]), bits(b[0]), err_msg=msg)
    np.testing.assert_array_equal(bits(a[2]), bits(b[2]), err_msg=msg)


# --------------------------------------------------------------------------------------------- 1. re-run
def test_run_lk_again_without_set_points(pkg, hip, frames, points):
    """single handle: run_lk runs whenever called, with the last points — the same bits twice.  Batch: run_lk runs only the slots
    armed by set_points, so the second call launches nothing and the first results stay readable."""
    t = pkg.TrackerHotpath(hip, **KW)
    b = pkg.TrackerBatch(hip, 1, **KW)
    try:
        t.push_image(frames[0]); t.push_image(frames[1]); t.set_points(points)
        t.prof_enable(True); t.prof_reset()
        t.run_lk(); first = t.get_lk()
        assert _launches(t).get("lk_track") == 1
        t.run_lk(); second = t.get_lk()
        assert _launches(t).get("lk_track") == 2
        _assert_lk_equal(first, second, "single handle, second run_lk")
        assert first[1].sum() > 0.5 * len(points)                      # the comparison is not between two failures

        b.push_images([frames[0]]); b.push_images([frames[1]]); b.set_points([points])
        b.prof_enable(True); b.prof_reset()
        b.run_lk(); bfirst = b.get_lk(0)
        assert _launches(b).get("lk_track") == 1
        b.run_lk(); bsecond = b.get_lk(0)
        assert _launches(b).get("lk_track") == 1
        _assert_lk_equal(bfirst, bsecond, "batch, second run_lk")
        _assert_lk_equal(bfirst, first, "batch against the single handle")
    finally:
        t.close(); b.close()


# --------------------------------------------------------------------------------------------- 2. zero points
def test_zero_points_launch_no_lk(pkg, hip, frames):
    none = np.zeros((0, 2), np.float32)
    t = pkg.TrackerHotpath(hip, **KW)
    b = pkg.TrackerBatch(hip, 1, **KW)
    try:
        t.push_image(frames[0]); t.push_image(frames[1])
        t.prof_enable(True); t.prof_reset()
        t.set_points(none); t.run_lk()
        xy, st, err = t.get_lk()
        assert len(xy) == 0 and len(st) == 0 and len(err) == 0
        assert "lk_track" not in _launches(t)

        b.push_images([frames[0]]); b.push_images([frames[1]])
        b.prof_enable(True); b.prof_reset()
        b.set_points([none]); b.run_lk()
        xy, st, err = b.get_lk(0)
        assert len(xy) == 0 and len(st) == 0 and len(err) == 0
        assert "lk_track" not in _launches(b)
    finally:
        t.close(); b.close()


# --------------------------------------------------------------------------------------------- 3. launch counts
def test_single_handle_launches_equal_a_one_slot_batch(pkg, hip, frames, points):
    """one full frame (push with equalize, LK, circles, run_gftt_async, finish_frame with a camera; no overflow): the same kernel
    names with the same launch counts on a single handle and on a one-slot batch.  163 x 117 builds levels 1 and 2 only."""
    t = pkg.TrackerHotpath(hip, **KW)
    b = pkg.TrackerBatch(hip, 1, **KW)
    try:
        t.set_equalize(True, 3.0, (8, 8)); b.set_equalize(True, 3.0, (8, 8))
        t.push_image(frames[0]); b.push_images([frames[0]])                # the pair exists before the counted frame
        t.prof_enable(True); t.prof_reset()
        b.prof_enable(True); b.prof_reset()

        t.push_image(frames[1]); t.set_points(points); t.run_lk()
        xy, st, _ = t.get_lk()
        k = xy[st == 1]
        kept = k[(k[:, 0] >= 0) & (k[:, 0] < W) & (k[:, 1] >= 0) & (k[:, 1] < H)]
        assert len(kept) > 10
        t.set_mask_circles(kept, 10); t.run_gftt_async(150 - len(kept))
        new, un = t.finish_frame(kept, CAM)

        b.push_images([frames[1]]); b.set_points([points]); b.run_lk()
        xyb, stb, _ = b.get_lk(0)
        np.testing.assert_array_equal(bits(xyb), bits(xy))
        b.set_mask_circles([kept], 10); b.run_gftt_async([150 - len(kept)])
        (newb, unb), = b.finish_frame([kept], [CAM])
        assert b.redo_mask() == 0
        np.testing.assert_array_equal(bits(newb), bits(new))
        assert len(new) > 0 and len(un) == len(kept) + len(new)

        single, batch = _launches(t), _launches(b)
        print("launches per frame:", single)
        assert single == batch
        assert single == {"clahe_lut": 1, "clahe_interp": 1, "pyrdown": 2, "lk_track": 1, "mask_fill": 1, "mask_circles": 1, "gftt_mineig": 1,
                          "gftt_count": 1, "gftt_emit": 1, "gftt_sortpick": 1, "frame_concat": 1, "mei_undistort": 1}
    finally:
        t.close(); b.close()
