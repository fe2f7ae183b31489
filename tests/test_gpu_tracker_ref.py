"""GPU tier (-m gpu): pyramidal LK and the min-eigenvalue map / corner selection of the HIP library against references that owe
nothing to the oracle (tests/tracker_ref.py, written from SURVEY App. A.6 / A.7), at windows, level counts, iteration limits,
epsilons and thresholds other than the defaults.  The bars and the scenes are those of tests/test_tracker_ref.py, where the oracle
is held to them on the CPU (tests/tracker_checks.py); E_orc, the oracle's own distance from the reference, is pinned there.

  1. exact step   one iteration from starts on the 1/64 grid: status equal, |x - (pt + delta*)| <= 2 ulp32(|pt| + win) + 16 2^-24 s;
                  zero iterations: the input bit for bit and err within 1 ulp
  2. runs, chains decidable (settled) points: status equal, |xy - xy_ref| <= max(4 E_orc, 4 ulp32)
  3. reload       the same bar on a scene whose points travel more than 8 px within the level (sJ is loaded again)
  4. batch        the 64 x 48 step scenes through lvi_tbatch_*, three slots, bit-equal to single handles
  5. map          |eig - ref| <= 2 u, u = 2^-24 ((a + c) + 2 sqrt(2 (a + c))); 0 where a + c = 0
  6. selection    good_features == gftt_select(the call's own TDBG_MINEIG) in order; TDBG_GFTT_NCAND equal
  7. tiny images  1x5 2x2 5x2: no corners; 3x3: what gftt_select returns"""
import numpy as np
import pytest

import tracker_checks as C
import tracker_scenes as SC
from helpers import bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", SC.STEP_NAMES)
def test_step_against_exact_reference(pkg, hip, name):
    rep = C.check_step(pkg, hip, C.scene(pkg, "step", name))
    print("hip step: worst share of the bar", rep["ratio"], "without the conditioning term", rep["ratio_round_only"], rep)
    if name.startswith("oblique"):
        assert rep["cond_max"] >= 1e3, rep


@pytest.mark.parametrize("name", SC.RUN_NAMES + SC.CHAIN_NAMES)
def test_runs_and_chains_against_reference(pkg, hip, name):
    kind = "run" if name in SC.RUN_NAMES else "chain"
    rep = C.check_run(pkg, hip, C.scene(pkg, kind, name), e_orc=C.E_ORC[name])
    print(f"hip {kind}: E = {rep['E']:.6g} px (E_orc {C.E_ORC[name]:.6g}), unsettled {rep['unsettled']}/{rep['n']}, "
          f"undecidable {rep['undecidable']}/{rep['n']};", rep)


def test_reload_of_the_resident_target_region(pkg, hip):
    scene = C.reload_scene()
    rep = C.check_run(pkg, hip, scene, e_orc=C.E_ORC[scene["name"]])
    print("hip reload:", rep)
    assert rep["travel_gt8"] >= 10, rep            # from the reference: the window leaves the resident region of its level


@pytest.mark.parametrize("win", (3, 15))
def test_batch_equals_single_handles_at_other_parameters(pkg, hip, win):
    """three slots on the 64 x 48 step scenes (slot 0 textured, slot 1 squeezed, slot 2 textured with the frames swapped), two
    rounds; slot 1 sits round 1 out.  One iteration at level 0, epsilon 0, as in item 1"""
    tex, sq = C.scene(pkg, "step", f"tex-64x48-win{win}"), C.scene(pkg, "step", f"squeezed-64x48-win{win}")
    pts = (tex["pts64"].astype(np.float64) / 64.0).astype(np.float32)
    frames = [(tex["I"], tex["J"]), (sq["I"], sq["J"]), (tex["J"], tex["I"])]
    kw = dict(max_width=64, max_height=48, max_features=256, lk_win=win, lk_max_level=0, lk_max_iters=1, lk_eps=0.0)
    singles = [pkg.TrackerHotpath(hip, **kw) for _ in range(3)]
    batch = pkg.TrackerBatch(hip, 3, **kw)
    try:
        batch.push_images([f[0] for f in frames])
        for t, f in zip(singles, frames):
            t.push_image(f[0])
        for rnd in (1, 2):
            out = [s == 1 and rnd == 1 for s in range(3)]
            nxt = [f[rnd % 2] for f in frames]                    # round 1: J, round 2: back to I
            p = [None if out[s] else (pts if rnd == 1 else pts[::-1].copy()) for s in range(3)]
            batch.push_images([None if out[s] else nxt[s] for s in range(3)])
            batch.set_points(p)
            batch.run_lk()
            for s, t in enumerate(singles):
                if out[s]:
                    continue
                t.push_image(nxt[s]); t.set_points(p[s]); t.run_lk()
                xb, sb, eb = batch.get_lk(s)
                xs, ss, es = t.get_lk()
                tag = f"win {win} round {rnd} slot {s}"
                assert len(xb) == len(pts) == len(xs), tag
                np.testing.assert_array_equal(sb, ss, err_msg=tag)
                np.testing.assert_array_equal(bits(xb), bits(xs), err_msg=tag)
                np.testing.assert_array_equal(bits(eb), bits(es), err_msg=tag)
                assert ss.sum() > 0, tag
    finally:
        for t in singles:
            t.close()
        batch.close()


@pytest.mark.parametrize("size", SC.MINEIG_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mineig_map_and_selection(pkg, hip, size):
    w, h = size
    t = pkg.TrackerHotpath(hip, max_width=max(w, 64), max_height=max(h, 64), max_features=4096)
    try:
        worst, ncases = {}, 0
        for name, img in SC.mineig_images(pkg.synth, w, h).items():
            _, worst[name] = C.check_mineig(t, pkg, img, (size, name))
            for (mk, q, md, quota) in SC.selection_cases(w, h, name):
                C.check_selection(t, pkg, img, SC.make_mask(mk, w, h), q, md, quota, (size, name, mk, q, md, quota))
                ncases += 1
        print(f"hip min-eigenvalue map {w}x{h}: worst |eig - ref| / u per image {worst}; {ncases} selections exact")
    finally:
        t.close()


@pytest.mark.parametrize("size", SC.TINY_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny_images(pkg, hip, oracle, size):
    """images without an interior (w < 3 or h < 3) have no candidates: zero corners on both libraries, and the map is still the
    float64 map to rounding; 3 x 3: whatever gftt_select makes of the library's own map"""
    w, h = size
    rng = np.random.default_rng(10 * w + h)
    imgs = [rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(250, 256, (h, w), dtype=np.uint8)]
    if size == (3, 3):
        imgs += [np.array(im, np.uint8) for im in SC.TINY_3X3]
    for lib in (oracle, hip):
        t = pkg.TrackerHotpath(lib, max_width=64, max_height=64, max_features=4096)
        try:
            for img in imgs:
                C.check_mineig(t, pkg, img, size)
                for (q, md, quota, mask) in ((0.01, 0.5, 0, None), (0.01, 1.0, 0, None), (0.3, 7.0, 1, np.ones((h, w), np.uint8))):
                    n, ncand = C.check_selection(t, pkg, img, mask, q, md, quota, size)
                    if w < 3 or h < 3:
                        assert n == 0 and ncand == 0, (size, n, ncand)
        finally:
            t.close()
