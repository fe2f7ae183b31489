"""GPU tier (-m gpu): the end of a Gauss-Newton iteration on the device (`icp_iter_end` in csrc/lvi_icp.hip: the QR solve on one
wavefront, the LDL^T shortcut, the Jacobi iteration, matP, the degenerate flag's way from launch to launch) against the
float64 reference tests/step_ref.py, on the scenes of tests/step_scenes.py.

Every recorded iteration is a problem of its own — 27 sums in (LVI_DBG_ICP_JTJ), one pose increment out (two rows of
LVI_DBG_ICP_POSE_TRACE) — so each library is judged on ITS OWN sums; the two need not have seen identical inputs.  The oracle's
deviation from float64, measured in the same run, is the yardstick: no constant tolerance in this file.

The scenes reach, on the device: degenerate == True with one direction removed (corridor, endwall_just_below) and with three
(slab: the `below = below && ...` chain, a rank-3 matP); the Jacobi iteration ending in NOT degenerate (endwall_in_zone:
lambda_min between 100 and the shortcut's 100 + 1e-4 trace); the shortcut (endwall_clear, boxes)."""
import numpy as np
import pytest

import step_ref
import step_scenes as S
from helpers import bits, small_params, xyzi

pytestmark = pytest.mark.gpu

VOX = {"vox_sorted": 1, "vox_binned": 2}
DEGENERATE_SCENES = [n for n in S.SCENE_NAMES if n in ("corridor", "endwall_just_below", "slab")]
_runs = {}


def runs(pkg, oracle, hip, name, mode, vox):
    """(oracle's match, HIP's match) of one scene on fresh handles, computed once per module and never modified"""
    sc = S.get(name, pkg, oracle)
    if ("orc", name, mode) not in _runs:
        _runs["orc", name, mode] = S.run(pkg, oracle, sc, **S.BREAK_SETTINGS[mode])
    if (vox, name, mode) not in _runs:
        _runs[vox, name, mode] = S.run(pkg, hip, sc, voxel_mode=VOX[vox], **S.BREAK_SETTINGS[mode])
    return sc, _runs["orc", name, mode], _runs[vox, name, mode]


@pytest.fixture(params=list(VOX))
def vox(request):
    return request.param


@pytest.fixture(params=list(S.BREAK_SETTINGS))
def mode(request):
    return request.param


# ----------------------------------------------------------------------------- 1. the step against float64, per side
@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_step_against_float64(pkg, oracle, hip, name, mode, vox):
    """E = |(trace[i+1] - trace[i]) - step64(jtj[i])| of every recorded iteration, rotation and translation apart:
    E_hip <= 4 max(E_orc_scene, U), E_orc_scene the oracle's largest E of the class over the scene's iterations, U the float32
    spacing at the largest pose component of the class.  4: two float32 restatements of QR and Jacobi that order their
    operations differently, at condition numbers of a few thousand.  A skipped or garbled projection misses by
    proj_gap >= 1e-3 (a precondition of every degenerate scene, asserted here on HIP's own sums): 4 - 5 orders above the bar."""
    sc, ro, rg = runs(pkg, oracle, hip, name, mode, vox)
    S.check_preconditions(sc, rg)
    S.check_preconditions(sc, ro)
    eo, eg = S.step_errors(ro), S.step_errors(rg)
    for k, cls in ((0, "rot"), (1, "trans")):
        cols = slice(0, 3) if k == 0 else slice(3, 6)
        u = step_ref.f32_spacing(np.abs(rg["trace"][:, cols]).max())
        e_orc, e_hip = eo[k].max(), eg[k].max()
        bar = 4 * max(e_orc, u)
        print(f"{name} {mode} {vox} {cls}: E_hip {e_hip:.3e}  E_orc {e_orc:.3e}  U {u:.3e}  bar {bar:.3e}  "
              f"lambda_min hip {eg[2][0].eigenvalues[0]:.3f} orc {eo[2][0].eigenvalues[0]:.3f}  proj_gap {eg[2][0].proj_gap:.3e}")
        assert e_hip <= bar, (name, mode, vox, cls, eg[k], bar)


# ----------------------------------------------------------------------------- 2. flags
@pytest.mark.parametrize("name", S.SCENE_NAMES)
def test_flags(pkg, oracle, hip, name, mode, vox):
    """degenerate / converged / iters = step_ref's verdict on HIP's own sums = the oracle's.  Decidable: lambda_min keeps
    0.5 from 100 (check_preconditions), no delta lies within 2 % of 0.05"""
    sc, ro, rg = runs(pkg, oracle, hip, name, mode, vox)
    S.check_preconditions(sc, rg)
    steps, degenerate, converged, iters = step_ref.replay(rg["jtj"], break_enabled=(mode == "break"))
    for s in steps:
        assert abs(s.delta_r - 0.05) > 1e-3 and abs(s.delta_t - 0.05) > 1e-3, (s.delta_r, s.delta_t)
    got = (rg["degenerate"], rg["converged"], rg["iters"])
    assert got == (degenerate, converged, iters), (name, got, (degenerate, converged, iters))
    assert got == (ro["degenerate"], ro["converged"], ro["iters"]), (name, got)
    assert rg["degenerate"] == sc["expect"]["degenerate"]
    assert rg["status"] == ro["status"] == 0
    if mode == "nobreak":
        assert rg["iters"] == 6


# ----------------------------------------------------------------------------- 3. the zero step
@pytest.mark.parametrize("name", DEGENERATE_SCENES)
def test_zero_step_after_the_first_iteration(pkg, oracle, hip, name, mode, vox):
    """the local matP is zero on iterations >= 1, a degenerate frame stops moving after iteration 0"""
    sc, ro, rg = runs(pkg, oracle, hip, name, mode, vox)
    assert rg["degenerate"]
    t = bits(rg["trace"])
    assert len(t) == rg["iters"] + 1
    assert (t[1:] == t[1]).all(), rg["trace"]
    assert (t[1] != t[0]).any(), "iteration 0 moves"
    np.testing.assert_array_equal(bits(rg["pose"]), t[1])
    assert rg["iters"] == (2 if mode == "break" else 6)
    assert rg["n_sel"][1:] == [rg["n_sel"][1]] * (rg["iters"] - 1)              # same pose, same rows


# ----------------------------------------------------------------------------- 4. the flag crosses launches, not frames
def test_degenerate_flag_across_frames(pkg, oracle, hip, mode, vox):
    """iteration 0's verdict is written by one launch and read at the entry of the following ones (`degen_in`); the next frame
    on the same handle must not inherit it"""
    cor, box = S.get("corridor", pkg, oracle), S.get("boxes", pkg, oracle)
    g = pkg.LidarHotpath(hip, voxel_mode=VOX[vox], **small_params(**S.BREAK_SETTINGS[mode]))
    out = []
    for sc in (cor, box, cor):
        S.load(g, sc)
        out.append(S.match(pkg, g, sc))
    g.close()
    a, b, c = out
    assert a["degenerate"] and c["degenerate"] and not b["degenerate"]
    assert (a["converged"], a["iters"], a["n_sel"]) == (c["converged"], c["iters"], c["n_sel"])
    np.testing.assert_array_equal(bits(a["pose"]), bits(c["pose"]))
    np.testing.assert_array_equal(bits(a["trace"]), bits(c["trace"]))
    np.testing.assert_array_equal(bits(a["jtj"]), bits(c["jtj"]))
    # and boxes in the middle is boxes on a fresh handle
    _, _, fresh = runs(pkg, oracle, hip, "boxes", mode, vox)
    assert b["iters"] == fresh["iters"] >= 3 and b["converged"] == fresh["converged"]
    np.testing.assert_array_equal(bits(b["pose"]), bits(fresh["pose"]))
    np.testing.assert_array_equal(bits(b["trace"]), bits(fresh["trace"]))


# ----------------------------------------------------------------------------- 5. the sums of iteration 0 against float64
def _own_sums(pkg, h, guess):
    """float64 AtA / AtB from the handle's own debug_residuals at `guess` + the number of flagged rows"""
    ori, cf = [], []
    for which in (0, 1):
        cloud = h.get_scan_ds()[which]
        co, fl = h.debug_residuals(which, guess)
        assert len(co) == len(cloud)
        ori.append(xyzi(cloud)[fl == 1, :3]); cf.append(xyzi(co)[fl == 1])
    ori, cf = np.concatenate(ori), np.concatenate(cf)
    return step_ref.normal_sums(ori, cf, guess) + (len(ori),)


@pytest.mark.parametrize("name", ["boxes", "corridor", "slab"])
def test_sums_of_iteration_zero_against_float64(pkg, oracle, hip, name, vox):
    """The same DS map and DS scan on both sides (HIP's, handed over as clouds of one point per voxel, as in
    test_residuals_at_fixed_pose).  The rows of iteration 0 rebuilt in float64 from debug_residuals' coefficients
    (mapOptimization.cpp:1225-1245), summed in float64, against jtj[0] of the same handle.  Bar, entry by entry:
    4 max(the oracle's own deviation, 2^-23 sum|terms|).  The oracle itself stays within 8 * 2^-23 sum|terms| (asserted; measured
    0.59 * 2^-23 sum|terms| at most, the device 0.70), i.e. debug_residuals and the match form the same coefficients there.

    boxes: every recorded iteration k, the rows rebuilt from debug_residuals at trace[k] against jtj[k], under the same bar.
    debug_residuals searches and fits afresh; iterations >= 1 of the match (`icp_gn_kernel`) skip the search where the feature
    has not moved beyond its bound and evaluate the fit stored by an earlier iteration.  The two must select the same rows
    (n_sel[k]) and form the same coefficients, or the sums differ."""
    A = pkg._abi
    sc = S.get(name, pkg, oracle)
    o = pkg.LidarHotpath(oracle, **small_params()); g = pkg.LidarHotpath(hip, voxel_mode=VOX[vox], **small_params())
    S.load(g, sc); S.match(pkg, g, sc)
    (mcg, msg), (scg, ssg) = g.get_map_ds(), g.get_scan_ds()
    res = {}
    for key, h in (("orc", o), ("hip", g)):
        h.map_set(mcg, msg)
        r = h.scan_to_map(scg, ssg, sc["guess"])
        jtj = h.debug_get(A.DBG_ICP_JTJ, np.float32).reshape(-1, 27)
        trace = h.debug_get(A.DBG_ICP_POSE_TRACE, np.float32).reshape(-1, 6)
        assert r["status"] == 0 and len(jtj) == r["iters"] and len(trace) >= r["iters"]
        np.testing.assert_array_equal(bits(trace[0]), bits(sc["guess"]))
        per_iter = []
        for k in (range(r["iters"]) if name == "boxes" else [0]):
            sums, terms, n_rows = _own_sums(pkg, h, trace[k])
            assert r["n_sel"][k] == n_rows >= 50, (key, k, r["n_sel"], n_rows)
            per_iter.append((np.abs(jtj[k].astype(np.float64) - sums), 2.0 ** -23 * terms))
        res[key] = (per_iter, r)
    o.close(); g.close()
    (it_orc, r_orc), (it_hip, r_hip) = res["orc"], res["hip"]
    assert len(it_orc) == len(it_hip) and (name != "boxes" or len(it_hip) == r_hip["iters"] == r_orc["iters"] >= 3)
    tiny = np.finfo(np.float64).tiny
    for k, ((d_orc, f_orc), (d_hip, f_hip)) in enumerate(zip(it_orc, it_hip)):
        assert r_orc["n_sel"][k] == r_hip["n_sel"][k]
        bar = 4 * np.maximum(d_orc, f_hip)
        print(f"{name} {vox} iteration {k}: rows {r_hip['n_sel'][k]}  D/F max: oracle {(d_orc / np.maximum(f_orc, tiny)).max():.3f}  "
              f"hip {(d_hip / np.maximum(f_hip, tiny)).max():.3f}  hip D/bar max {(d_hip / np.maximum(bar, tiny)).max():.3f}")
        assert (d_orc <= 8 * f_orc).all(), (k, d_orc, f_orc)
        assert (d_hip <= bar).all(), (k, d_hip, bar)
