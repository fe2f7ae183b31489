"""CPU tier: the tracker references (tests/tracker_ref.py, written from SURVEY App. A.6 / A.7) against closed forms, and the
oracle against the references at every bar the GPU tier applies to the HIP library (tests/test_gpu_tracker_ref.py).  Each class
prints what it measured: E_orc (the oracle's greatest distance from the reference), the unsettled and the undecidable share.

Measured on 2026-10-19 (DESIGN "Tracker references"; pinned in tracker_checks.E_ORC / ORC_*):
  step: status equal on all 1 418 starts, err within 0.50 ulp, position within 0.376 of its bar (0.75 ulp), conditioning up to 7.8e3;
  runs: 0 undecidable, 0-3 of 80 unsettled, E_orc 0 ... 1.4e-3 px; chains 3.1e-5 ... 2.8e-3 px; reload 1.3e-3 px, 57 of 64 points
  travel more than 8 px; min-eigenvalue map within 0.595 u; selection exact in all 600 cases."""
import numpy as np
import pytest

import tracker_checks as C
import tracker_ref as R
import tracker_scenes as SC


# ----------------------------------------------------------------------------- the reference against closed forms
def _scharr_loops(img, x, y):
    """Scharr at an interior pixel by the definition, nothing shared with tracker_ref.scharr"""
    k = ((-3, 0, 3), (-10, 0, 10), (-3, 0, 3))
    gx = sum(k[j][i] * int(img[y + j - 1, x + i - 1]) for j in range(3) for i in range(3))
    gy = sum(k[i][j] * int(img[y + j - 1, x + i - 1]) for j in range(3) for i in range(3))
    return gx, gy


def test_identical_frames_give_no_step_and_no_error(pkg):
    img = pkg.synth.make_texture(97, 61, 3)
    for win in (3, 7, 21):
        for q in ((64 * 40, 64 * 30), (64 * 50 + 17, 64 * 20 + 63), (5, 64 * 59 + 1)):
            r = R.lk_step_exact(img, img, q, win)
            assert r["status"] == 1 and r["delta"] == (0.0, 0.0) and r["err"] == 0.0 and r["sums"][3:] == (0, 0)


def test_brightness_offset_gives_b_in_closed_form(pkg):
    """J = I + c without saturation: every patch difference is exactly 32 c (the weights add up to 2^14), so at a whole-pixel
    start b1 = 32 c * sum of the Scharr x-derivatives of the window, b2 likewise"""
    img = (40 + (pkg.synth.make_texture(97, 61, 5).astype(np.int32) * 150) // 255).astype(np.uint8)
    for win, (x, y), c in ((5, (30, 20), 7), (21, (48, 30), 3), (7, (11, 40), 60)):
        r = R.lk_step_exact(img, (img + c).astype(np.uint8), (64 * x, 64 * y), win)
        half = (win - 1) // 2
        g = [_scharr_loops(img, xx, yy) for yy in range(y - half, y + half + 1) for xx in range(x - half, x + half + 1)]
        assert r["sums"][3] == 32 * c * sum(a for a, _ in g) and r["sums"][4] == 32 * c * sum(b for _, b in g)
        assert r["sums"][:3] == (sum(a * a for a, _ in g), sum(a * b for a, b in g), sum(b * b for _, b in g))
        assert r["err"] == 32.0 * c * win * win / (32.0 * win * win)
        # off the pixel grid the difference is still 32 c everywhere
        r = R.lk_step_exact(img, (img + c).astype(np.uint8), (64 * x + 21, 64 * y + 40), win)
        assert r["err_sum"] == 32 * c * win * win


def test_ramp_derivative_and_one_pixel_shift():
    """rows that are ramps of slope g have the Scharr derivative (32 g, .) everywhere inside; with a kink down the columns the
    system is regular and a shift of the content by one pixel gives the step (1, 0) exactly:
    b = -32 g (sum Ix, sum Iy) = -(A11, A12) since Ix = 32 g, and A^-1 (A11, A12)^T = (1, 0)^T"""
    h, w, g, k, cy = 48, 64, 2, 3, 24
    yy, xx = np.mgrid[0:h, 0:w]
    img = (10 + g * xx + k * np.maximum(yy - cy, 0)).astype(np.uint8)
    assert img.max() < 255
    dx, dy = R.scharr(img)
    assert (dx[:, 1:-1] == 32 * g).all() and (dx[:, 0] == 0).all() and (dx[:, -1] == 0).all()
    flat = np.broadcast_to((10 + g * np.arange(w)).astype(np.uint8), (h, w))
    fx, fy = R.scharr(flat)
    assert (fx[:, 1:-1] == 32 * g).all() and (fy == 0).all()
    v = {cy - 1: 0, cy: 16 * k}                                   # Scharr dy = 16 (I[y+1] - I[y-1]) on rows of equal slope
    shifted = np.empty_like(img); shifted[:, 1:] = img[:, :-1]; shifted[:, 0] = img[:, 0]
    for win, x0 in ((7, 30), (21, 32), (5, 20)):
        half = (win - 1) // 2
        r = R.lk_step_exact(img, shifted, (64 * x0, 64 * cy), win)
        rows = [v.get(y, 0 if y < cy else 32 * k) for y in range(cy - half, cy + half + 1)]
        s11, s12, s22 = win * win * (32 * g) ** 2, 32 * g * win * sum(rows), win * sum(t * t for t in rows)
        assert r["sums"] == (s11, s12, s22, -s11, -s12)
        assert r["delta"] == (1.0, 0.0) and r["status"] == 1
        assert r["err"] == g                                      # |J - I| = g grey levels at every pixel


def test_weights_and_reflection():
    assert R.weights_f32(0.0, 0.0) == (1 << 14, 0, 0, 0)
    assert R.weights_f32(0.5, 0.5) == (4096, 4096, 4096, 4096)
    # 1/3, 1/3 in float32: 7281.78 7281.78 -> 7282 each, 3640.89 -> left as the remainder 16384 - 7282 - 3641 - 3641 = 1820
    w = R.weights_f32(np.float32(2) / np.float32(3), np.float32(2) / np.float32(3))
    assert w == (1820, 3641, 3641, 16384 - 1820 - 2 * 3641)
    np.testing.assert_array_equal(R.reflect_idx(np.arange(-7, 8), 3), [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1])
    np.testing.assert_array_equal(R.reflect_idx(np.arange(-2, 3), 1), 0)
    # the stop rule of buildOpticalFlowPyramid: 160 x 120, window 21, three levels asked, two reached
    assert [a.shape for a in R.build_pyramid(np.zeros((120, 160), np.uint8), 21, 3)] == [(120, 160), (60, 80), (30, 40)]
    assert len(R.build_pyramid(np.zeros((18, 24), np.uint8), 7, 1)) == 2 and len(R.build_pyramid(np.zeros((517, 643), np.uint8), 3, 7)) == 8


def test_mineig_closed_forms():
    img = np.zeros((20, 30), np.uint8); img[:, 15:] = 200                # a vertical edge: Dy = 0, one eigenvalue is zero
    e, apc = R.mineig_ref(img)
    assert (e == 0).all() and apc.max() > 0
    # one pixel of 255 on black: Dx, Dy around it are the flipped Sobel kernels times 255, so at the pixel itself
    # sum Dx^2 = sum Dy^2 = 12 * 255^2, sum Dx Dy = 0, a = c = 6 * (255 / 3060)^2 = 1 / 24 and the eigenvalue is 2 a = 1 / 12
    img = np.zeros((9, 9), np.uint8); img[4, 4] = 255
    e, apc = R.mineig_ref(img)
    assert abs(e[4, 4] - 1.0 / 12.0) < 1e-16 and abs(apc[4, 4] - 1.0 / 12.0) < 1e-16
    # one pixel to the right the box holds the columns 0, +1 (and +2, empty) of those kernels: sum Dx^2 = (1 + 4 + 1) 255^2,
    # sum Dy^2 = (4 + 4 + 1 + 1) 255^2, sum Dx Dy = (-1 + 1) 255^2 = 0: a = 3 / 144, c = 5 / 144, eigenvalue 8 / 144 - 2 / 144 = 1 / 24
    assert abs(e[4, 5] - 1.0 / 24.0) < 1e-16 and abs(apc[4, 5] - 8.0 / 144.0) < 1e-16
    assert abs(e[5, 5] - e[3, 3]) == 0 and e[5, 5] > 0                   # the four diagonal neighbours are alike


def test_gftt_select_rules():
    e = np.zeros((7, 9), np.float32)
    e[2, 2] = e[2, 6] = e[4, 4] = 5.0          # three equal maxima
    e[3, 3] = 4.5                              # next to two of them: not its neighbourhood's maximum
    e[5, 7] = 4.0                              # a weaker maximum of its own
    e[1, 7] = 0.04                             # below thr = 9 * 0.01
    e[0, 4] = 9.0                              # on the border: never a candidate, but it sets the threshold
    xy, n = R.gftt_select(e, None, 0.01, 0.5, 0)
    assert n == 4 and xy.tolist() == [[4, 4], [6, 2], [2, 2], [7, 5]]                          # equal values: higher address first
    assert R.gftt_select(e, None, 0.01, 2.82, 0)[0].tolist() == [[4, 4], [6, 2], [2, 2], [7, 5]]   # 8 >= 2.82^2
    assert R.gftt_select(e, None, 0.01, 2.9, 0)[0].tolist() == [[4, 4], [7, 5]]                # 8 < 2.9^2 drops both; (7, 5): 9 + 1 from (4, 4)
    assert R.gftt_select(e, None, 0.01, 3.2, 0)[0].tolist() == [[4, 4]]                        # 10 < 10.24
    m = np.zeros((7, 9), np.uint8); m[2, 2] = m[1, 7] = 1
    assert R.gftt_select(e, m, 0.01, 0.5, 0)[0].tolist() == [[2, 2]]                           # the maximum is taken under the mask: thr = 0.05
    m[1, 7] = 0; m[5, 7] = 3
    assert R.gftt_select(e, m, 0.9, 0.5, 0)[0].tolist() == [[2, 2]]                            # 4 <= 0.9 * 5
    assert R.gftt_select(e, None, 0.01, 0.5, 2)[0].tolist() == [[4, 4], [6, 2]]
    assert R.gftt_select(e, None, 0.01, 5.0, 1)[0].tolist() == [[4, 4]]
    for shape in ((5, 1), (2, 2), (2, 5), (1, 1)):
        assert R.gftt_select(np.ones(shape, np.float32), None, 0.01, 1.0, 0)[1] == 0           # no interior
    assert R.gftt_select(np.ones((3, 3), np.float32), None, 0.01, 1.0, 0)[0].tolist() == [[1, 1]]


# ----------------------------------------------------------------------------- the oracle against the reference
@pytest.mark.parametrize("name", SC.STEP_NAMES)
def test_oracle_step(pkg, oracle, name):
    rep = C.check_step(pkg, oracle, C.scene(pkg, "step", name))
    print("oracle step:", rep)
    assert rep["ratio"] <= C.ORC_STEP_RATIO and rep["err_ulp"] <= C.ORC_ERR_ULP, rep
    if name.startswith("oblique"):
        assert rep["cond_max"] >= 1e3 and rep["ratio_round_only"] > 1.0, rep          # the scene does exercise the conditioning term


@pytest.mark.parametrize("name", SC.RUN_NAMES + SC.CHAIN_NAMES + ["reload-blobs"])
def test_oracle_run(pkg, oracle, name):
    kind = "run" if name in SC.RUN_NAMES else "chain"
    scene = C.reload_scene() if name == "reload-blobs" else C.scene(pkg, kind, name)
    rep = C.check_run(pkg, oracle, scene)
    print(f"oracle {kind}: E_orc = {rep['E']:.6g} px, unsettled {rep['unsettled']}/{rep['n']}, undecidable {rep['undecidable']}/{rep['n']};", rep)
    assert rep["E"] <= C.E_ORC[name], (rep, C.E_ORC[name])                             # the pin of the measured figure
    if name == "reload-blobs":
        assert rep["travel_gt8"] >= 10, rep                                            # otherwise the scene does not reach the reload
    # the oracle passes the device's own bar a fortiori
    C.check_run(pkg, oracle, scene, e_orc=C.E_ORC[name])


@pytest.mark.parametrize("size", SC.MINEIG_SIZES + SC.TINY_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_mineig_and_selection(pkg, oracle, size):
    w, h = size
    t = pkg.TrackerHotpath(oracle, max_width=max(w, 64), max_height=max(h, 64), max_features=4096)
    try:
        if size in SC.TINY_SIZES:
            rng = np.random.default_rng(10 * w + h)
            for img in (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(250, 256, (h, w), dtype=np.uint8)):
                _, ratio = C.check_mineig(t, pkg, img, size)
                assert ratio <= C.ORC_MINEIG_RATIO
                if w < 3 or h < 3:
                    assert len(t.good_features(img, 0, 0.01, 1.0)) == 0
                else:
                    C.check_selection(t, pkg, img, None, 0.01, 0.5, 0, size)
            return
        worst, ncases = {}, 0
        for name, img in SC.mineig_images(pkg.synth, w, h).items():
            _, worst[name] = C.check_mineig(t, pkg, img, (size, name))
            for (mk, q, md, quota) in SC.selection_cases(w, h, name):
                C.check_selection(t, pkg, img, SC.make_mask(mk, w, h), q, md, quota, (size, name, mk, q, md, quota))
                ncases += 1
        print(f"oracle min-eigenvalue map {w}x{h}: worst |eig - ref| / u per image {worst}; {ncases} selections exact")
        assert max(worst.values()) <= C.ORC_MINEIG_RATIO, worst
    finally:
        t.close()


def test_tiny_3x3_selection(pkg, oracle):
    """3 x 3 images, where the only interior pixel is the only possible corner: the selection must be what gftt_select makes of the
    library's own map (by reflection the centre's value never exceeds its ring's, so a corner needs an exact tie)"""
    t = pkg.TrackerHotpath(oracle, max_width=64, max_height=64, max_features=4096)
    got = [C.check_selection(t, pkg, np.array(im, np.uint8), None, 0.01, 1.0, 0, "3x3") for im in SC.TINY_3X3]
    t.close()
    assert got[0] == (0, 0) and all(g in ((0, 0), (1, 1)) for g in got)
