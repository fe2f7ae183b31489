"""GPU tier of the initial two-view pose (include/lvi_relpose.h) against tests/relpose_ref.py.  recover is
equality of bits: every field of the pose, the four candidates and the four masks, with nothing set aside.  solve and find
hold the sample stream and the status of the owned RANSAC as test_gpu_fmat.py holds them (the stream bit for bit, the walk
replayed from the device's scores, the status from the device's own F) and from there on are equality of bits again, with
the reference fed the device's own F and status (DESIGN §11 says why F itself agrees only to rounding)."""
import os
import subprocess

import numpy as np
import pytest

import fman_ref as FM
import fmat_ref
import relpose_ref as R

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257]
MAXP = 257


@pytest.fixture(scope="module")
def rp(pkg, hip):
    h = pkg.RelativePose(hip, max_points=MAXP)
    yield h
    h.close()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _assert_pose(dev, ref, where):
    for k in ("R", "t", "sv"):
        assert np.array_equal(_bits(dev[k]).ravel(), _bits(ref[k]).ravel()), (where, k)
    assert (dev["good"], dev["chosen"], dev["n_inliers"], dev["flags"], dev["sweeps"]) == \
        (ref["good"], ref["chosen"], ref["n_inliers"], ref["flags"], ref["sweeps"]), where


def _assert_recover(rp, s, ref, where, mask="scene"):
    """one device recover against a reference result: pose, chosen mask, the four candidates, the four masks"""
    m = s["mask"] if isinstance(mask, str) else mask
    dev = rp.recover(s["E"], s["p1"], s["p2"], m, s.get("dist", R.DIST))
    _assert_pose(dev, ref, where)
    assert np.array_equal(dev["mask"], ref["mask"]), where
    cand, masks = rp.last()
    for c in range(4):
        assert np.array_equal(_bits(cand[c][0]).ravel(), _bits(ref["cand"][c][0]).ravel()) and np.array_equal(_bits(cand[c][1]), _bits(ref["cand"][c][1])), (where, c)
    assert np.array_equal(masks, ref["masks"]), where
    return dev


_size_cache = {}


def _size_scene(n):
    """an exact scene of n points (even n) or a 7-point F with n of its points (odd n), and the reference without a mask"""
    if n not in _size_cache:
        if n % 2 == 0:
            p1, p2, _, _, E, _ = R.two_view(300 + n, n)
        else:
            f = R.scenes()["fmat21"]
            p1, p2, E = np.resize(f["p1"], (n, 2)), np.resize(f["p2"], (n, 2)), f["E"]
        s = dict(E=E, p1=p1, p2=p2, mask=None)
        _size_cache[n] = (s, R.recover(E, p1, p2))
    return _size_cache[n]


@pytest.mark.parametrize("n", SIZES)
def test_recover_equals_the_reference_bit_for_bit(rp, n):
    s, ref = _size_scene(n)
    _assert_recover(rp, s, ref, ("null", n))
    some = (np.random.RandomState(n).uniform(size=n) < 0.6).astype(np.uint8) * 3          # any non-zero byte means "use"
    _assert_recover(rp, s, R.with_mask(ref, some), ("mask", n), some)
    dev = _assert_recover(rp, s, R.with_mask(ref, np.zeros(n)), ("zeros", n), np.zeros(n, np.uint8))
    assert dev["chosen"] == 0 and dev["n_inliers"] == 0
    print(f"[relpose gpu] n {n}: counts {ref['good']}, chosen {ref['chosen']}, sweeps {ref['sweeps']}")


def test_recover_on_a_handle_of_fifteen(pkg, hip):
    h = pkg.RelativePose(hip, max_points=15)
    try:
        p1, p2, _, _, E, _ = R.two_view(315, 15)
        s = dict(E=E, p1=p1, p2=p2, mask=None)
        _assert_recover(h, s, R.recover(E, p1, p2), "max_points 15")
        with pytest.raises(pkg.LviError) as e:
            h.recover(E, np.resize(p1, (16, 2)), np.resize(p2, (16, 2)))
        assert e.value.code == pkg._abi.LVI_ERR_INVALID_ARG
    finally:
        h.close()


def test_recover_on_every_scene_and_branch(rp):
    winners = set()
    for name, s in R.scenes().items():
        ref = R.recover(s["E"], s["p1"], s["p2"], s["mask"])
        _assert_recover(rp, s, ref, name)
        winners.add(ref["chosen"])
    assert winners == {0, 1, 2, 3}
    for name, s in R.branch_scenes().items():
        ref = R.recover(s["E"], s["p1"], s["p2"], s["mask"], s["dist"])
        dev = _assert_recover(rp, s, ref, name)
        assert np.isfinite(dev["R"]).all() and np.isfinite(dev["t"]).all(), name
        if name.startswith("E_") and name not in ("E_outer", "E_neg", "E_small"):
            assert dev["flags"] == R.FLAG_DEGENERATE and (dev["R"] == np.eye(3)).all() and not dev["t"].any() and dev["good"] == [0, 0, 0, 0]
    for k in (12, 13):
        pairs, status, E = R.inlier_scene(k)
        p1, p2 = R.pair_points(pairs)
        dev = _assert_recover(rp, dict(E=E, p1=p1, p2=p2, mask=status), R.recover(E, p1, p2, status), f"inliers{k}")
        assert dev["n_inliers"] == k


def test_a_point_does_not_depend_on_its_slot_or_its_neighbours(rp):
    s, ref = _size_scene(64)
    big, _ = _size_scene(256)
    p1, p2 = big["p1"].copy(), big["p2"].copy()
    p1[:40], p2[:40] = s["p1"][:40], s["p2"][:40]
    p1[200:240], p2[200:240] = s["p1"][:40], s["p2"][:40]
    rp.recover(s["E"], p1, p2)
    _, masks = rp.last()
    assert np.array_equal(masks[:, :40], masks[:, 200:240]) and np.array_equal(masks[:, :40], ref["masks"][:, :40])
    a = rp.recover(s["E"], p1, p2)
    first = (a, rp.last())
    b = rp.recover(s["E"], p1, p2)
    second = (b, rp.last())
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert np.array_equal(first[1][1], second[1][1]) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(first[1][0], second[1][0]))


# ---- solve ------------------------------------------------------------------------------------------------------
def _hold_ransac(rp, out, p1, p2):
    """test_gpu_fmat.py's hold on one call of the owned RANSAC: the sample stream bit for bit, every score the reference's
    error function on the device's own F, the walk replayed from the device's scores, the status from the device's own F"""
    info, thr = out["info"], R.THRESHOLD
    tr = rp.fmat().trace()
    path, n = info["path"], len(p1)
    subs, niters0 = fmat_ref.sample_stream(p1, p2, n, path, 1000, R.CONFIDENCE, 1)
    assert info["n_subsets"] == len(subs)
    assert np.array_equal(tr["subsets"], np.array(subs, np.int32).reshape(-1, 7))
    run = min(info["iters"], info["n_subsets"])
    for h in range(run):
        for m in range(int(tr["nmodels"][h])):
            assert int(tr["score"][h, m]) == fmat_ref.score_candidates(path, tr["F"][h, m].ravel(), p1, p2, thr), (h, m)
    it, bi, br, bmed = fmat_ref.walk(path, n, niters0, info["n_subsets"], tr["nmodels"], tr["score"], R.CONFIDENCE)
    assert (it, bi, br) == (info["iters"], info["best_iter"], info["best_root"])
    Fd = tr["F"][bi, br].ravel() if bi >= 0 else np.zeros(9)
    assert np.array_equal(info["F"].ravel(), Fd)
    assert np.array_equal(out["status"], fmat_ref.final_mask(path, n, Fd, bi, bmed, p1, p2, thr))
    assert info["n_inliers"] == int(out["status"].sum())


def _assert_solve(rp, pairs, where):
    out = rp.solve(pairs)
    p1, p2 = R.pair_points(pairs)
    assert out["average_parallax"] == (R.average_parallax(pairs) if len(pairs) else 0.0), where
    if len(pairs) < R.MIN_PAIRS_SOLVE:
        assert not out["ok"] and out["flags"] == R.FLAG_TOO_FEW and (out["Rotation"] == np.eye(3)).all() and not out["Translation"].any() and not out["status"].any()
        return out
    _hold_ransac(rp, out, p1, p2)
    ref = R.solve_relative_rt(pairs, model=(out["status"], out["info"]["F"], out["info"]["best_iter"]))
    assert (out["ok"], out["flags"]) == (ref["ok"], ref["flags"]), where
    assert np.array_equal(_bits(out["Rotation"]).ravel(), _bits(ref["Rotation"]).ravel()) and np.array_equal(_bits(out["Translation"]), _bits(ref["Translation"])), where
    if ref["pose"] is not None:
        _assert_pose(out["pose"], ref["pose"], where)
        cand, masks = rp.last()
        assert np.array_equal(masks, ref["pose"]["masks"]), where
    return out


@pytest.mark.parametrize("n", [14, 15, 16, 150])
@pytest.mark.parametrize("outliers", [0.0, 0.3])
def test_solve_equals_the_reference_on_the_devices_own_model(rp, n, outliers):
    p1, p2, Rm, t, *_ = R.two_view(500 + n, n, noise=0.1 / R.FOCAL, outliers=outliers)
    out = _assert_solve(rp, R.pairs_of(p1, p2), (n, outliers))
    print(f"[relpose gpu] solve n {n} outliers {outliers}: ok {out['ok']}, RANSAC inliers {out['info']['n_inliers']}, pose inliers {out['pose']['n_inliers']}, "
          f"counts {out['pose']['good']}, iterations {out['info']['iters']}")
    if n == 150:                                                     # 105 pairs or more within a third of the threshold's noise: far beyond 12
        assert out["ok"] and np.abs(out["Rotation"] - Rm.T).max() < 2e-2                           # it is the motion, inverted


def test_solve_without_a_model(rp):
    k = np.arange(40)
    p1 = np.c_[(50 + 8 * k) / 460.0, (100 + 2 * k) / 460.0]
    out = _assert_solve(rp, R.pairs_of(p1, p1 + 3 / 460.0), "collinear")
    assert out["flags"] == R.FLAG_NO_MODEL and not out["ok"] and out["info"]["best_iter"] == -1 and not out["status"].any()
    assert (out["Rotation"] == np.eye(3)).all() and not out["Translation"].any() and out["pose"]["good"] == [0, 0, 0, 0]


# ---- find ---------------------------------------------------------------------------------------------------------
def _device_window(pkg, hip, kind):
    tab = pkg.FeatureTable(hip, max_features=64)
    FM.load(tab, R.window_frames(kind))
    return tab


def _assert_find(rp, tab, kind):
    ok, l, Rot, T, recs = rp.find(tab)
    solved = iter([r for r in recs if r["solved"]])

    def solve(pairs):
        d = next(solved)["result"]
        _hold_ransac_light(d, pairs)
        return R.solve_relative_rt(pairs, model=(d["status"], d["info"]["F"], d["info"]["best_iter"]))

    fm = FM.FeatureManager()
    FM.load(fm, R.window_frames(kind))
    rok, rl, rRot, rT, rrecs = R.relative_pose(fm.corresponding, solve=solve)
    assert (ok, l) == (rok, rl), kind
    assert np.array_equal(_bits(Rot).ravel(), _bits(rRot).ravel()) and np.array_equal(_bits(T), _bits(rT)), kind
    assert [(r["frame"], r["n"], r["average_parallax"], r["solved"], r["ok"]) for r in recs] == \
        [(r["frame"], r["n"], r["average_parallax"], r["solved"], r["ok"]) for r in rrecs], kind
    return ok, l, Rot, T, recs


def _hold_ransac_light(d, pairs):
    """the status is the reference's final mask on the device's own F (the stream and the walk are held in the solve tests)"""
    p1, p2 = R.pair_points(pairs)
    info = d["info"]
    assert info["path"] == "ransac" and info["best_iter"] >= 0
    assert np.array_equal(d["status"], fmat_ref.final_mask("ransac", len(p1), info["F"].ravel(), info["best_iter"], 0.0, p1, p2, R.THRESHOLD))


@pytest.mark.parametrize("kind", R.WINDOWS)
def test_find_equals_the_reference_loop(pkg, hip, rp, kind):
    tab = _device_window(pkg, hip, kind)
    try:
        ok, l, Rot, T, recs = _assert_find(rp, tab, kind)
    finally:
        tab.close()
    want = dict(first=(True, 0), third=(True, 3), garbage=(True, 3), still=(False, -1), pairs20=(False, -1), pairs21=(True, 0), below=(False, -1), above=(True, 0))
    assert (ok, l) == want[kind]
    print(f"[relpose gpu] find {kind}: ok {ok}, l {l}, frames visited {len(recs)}, solves {sum(r['solved'] for r in recs)}")


def test_cpp_mirror_equals_the_python_class(pkg, hip, rp, tmp_path):
    """lvi_host::MotionEstimator and lvi_host::relativePose over lvi_host::FeatureManager, through a small driver"""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.dirname(pkg.HIP_LIB_PATH)
    exe = tmp_path / "relpose_mirror"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(pkg.PKG_DIR, "host"), "-o", str(exe),
                        os.path.join(here, "relpose_mirror_driver.cpp"), "-L" + csrc, "-llvi_hip", "-Wl,-rpath," + csrc], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    kinds = ("third", "garbage", "still", "pairs20", "above")
    blob, want = np.array([float(MAXP), float(len(kinds))]).tobytes(), []
    for kind in kinds:
        for ids, obs in R.window_frames(kind):
            blob += np.array([float(len(ids))]).tobytes() + np.c_[np.asarray(ids, np.float64), np.asarray(obs, np.float64).reshape(-1, 8)].tobytes()
        tab = _device_window(pkg, hip, kind)
        try:
            ok, l, Rot, T, recs = rp.find(tab)
        finally:
            tab.close()
        last = [r for r in recs if r["solved"]]
        tail = [float(last[-1]["result"]["flags"]), float(last[-1]["result"]["pose"]["n_inliers"]), float(last[-1]["result"]["pose"]["chosen"]),
                last[-1]["result"]["average_parallax"]] if last else [0.0, 0.0, 0.0, 0.0]
        want.append(np.r_[float(ok), float(l), Rot.ravel(), T, tail])
    (tmp_path / "in.bin").write_bytes(blob)
    out = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.float64).reshape(len(kinds), 18)
    for kind, g, w in zip(kinds, got, want):
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), kind


# ---- errors and lifecycle -------------------------------------------------------------------------------------------
def test_errors_leave_the_last_result_readable(pkg, hip, rp):
    A = pkg._abi
    s, ref = _size_scene(64)
    rp.recover(s["E"], s["p1"], s["p2"])
    before = rp.last()
    big1, big2 = np.zeros((MAXP + 1, 2), np.float32), np.zeros((MAXP + 1, 2), np.float32)
    for call in (lambda: rp.recover(s["E"], big1, big2), lambda: rp.recover(s["E"], big1[:0], big2[:0]),
                 lambda: rp.recover(s["E"], s["p1"], s["p2"], None, 0.0), lambda: rp.recover(s["E"], s["p1"], s["p2"], None, float("nan")),
                 lambda: rp.solve(np.zeros((MAXP + 1, 6))), lambda: rp.set_params(threshold=0.0), lambda: rp.set_params(confidence=1.0),
                 lambda: rp.set_params(distance_thresh=-1.0)):
        with pytest.raises(pkg.LviError) as e:
            call()
        assert e.value.code == A.LVI_ERR_INVALID_ARG
    lib = rp.lib
    res = pkg.relpose.RelposeResult()
    assert lib.dll.lvi_relpose_solve(rp._h, None, -1, res, None) == A.LVI_ERR_INVALID_ARG
    assert lib.dll.lvi_relpose_solve(rp._h, None, 3, res, None) == A.LVI_ERR_INVALID_ARG
    after = rp.last()
    assert np.array_equal(before[1], after[1]) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(before[0], after[0]))
    assert np.array_equal(after[1], ref["masks"])
    assert (rp.params.threshold, rp.params.confidence, rp.params.distance_thresh) == (R.THRESHOLD, R.CONFIDENCE, R.DIST)
    # fewer than fifteen pairs is an answer, not an error, and it leaves the last recover alone as well
    out = rp.solve(np.zeros((0, 6)))
    assert not out["ok"] and out["flags"] == R.FLAG_TOO_FEW and np.array_equal(rp.last()[1], ref["masks"])
    fresh = pkg.RelativePose(hip, max_points=32)
    try:
        with pytest.raises(pkg.LviError) as e:
            fresh.last()
        assert e.value.code == A.LVI_ERR_STATE
    finally:
        fresh.close()


def test_create_rejects_sizes_out_of_range_and_survives_twenty_rounds(pkg, hip):
    for bad in (dict(max_points=14), dict(max_points=pkg.relpose.MAX_POINTS + 1), dict(max_iters=0), dict(max_iters=4097)):
        with pytest.raises(pkg.LviError) as e:
            pkg.RelativePose(hip, **bad)
        assert e.value.code == pkg._abi.LVI_ERR_INVALID_ARG
    s, ref = _size_scene(64)
    for k in range(20):
        h = pkg.RelativePose(hip, max_points=64 + k)
        try:
            if k % 5 == 0:
                _assert_recover(h, s, ref, ("round", k))
        finally:
            h.close()
