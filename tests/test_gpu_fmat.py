"""GPU tier of the device RANSAC (include/lvi_fmat.h) against the host restatement tests/fmat_ref.py, call
for call: the sample stream bit for bit, every candidate's score against the reference's error function on the device's
own F, the walk replayed from the device's scores, F to 1e-9 relative where the cubic is well conditioned, and the final
status, with every difference classified.  Besides the two classes of the contract (a candidate F beyond 1e-9, an error
within 4 f32 ulp of the threshold) there is a third: LMeDS at n <= 13, whose medians are rounding noise, so a last-bit
difference of one candidate's F can change the winner (fmat_ref.lmeds_rounding_decided); it is counted and bounded on its
own rather than against the 1 % budget."""

import numpy as np
import pytest

import fmat_ref as R

pytestmark = pytest.mark.gpu

F_RTOL = 1e-9
KAPPA_CUT = 1e-10          # predicted relative F change under a 16-ulp root perturbation above which F is "ill conditioned"
ULP_BAND = 4               # f32 ulps around the threshold within which a status difference is explained

NS = [8, 11, 14, 15, 16, 150, 1000, 2500]
OUTLIERS = [0.0, 0.1, 0.3, 0.5]


def _cases():
    out = []
    for seed in range(10):
        for n in NS:
            for o in OUTLIERS:
                out.append((n, o, "general", seed))
    for kind in ("rotation", "planar", "zero", "duplicates", "collinear"):
        for seed in range(2):
            for n in NS:
                out.append((n, 0.3 if kind != "zero" else 0.0, kind, 100 + seed))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def fr(pkg, hip):
    h = pkg.FundamentalRansac(hip, max_points=2500, max_iters=1000)
    yield h
    h.close()


def _relF(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    s = max(np.abs(b).max(), 1e-300)
    d = np.abs(a - b).max()
    return 0.0 if d == 0 else (np.inf if not np.isfinite(d) else d / s)


def _kappa(p1, p2, idx):
    """the largest relative change of a reference candidate F when its root moves by 16 ulp (of max(|root|, 1)): the
    sensitivity of F to the only steps that are not IEEE operations (acos, cos, pow of solveCubic)"""
    cands, roots, f1, f2 = R.run7point(p1[idx], p2[idx], with_roots=True)
    worst = 0.0
    for F, r in zip(cands, roots):
        dr = 16 * 2.0 ** -52 * max(abs(r), 1.0)
        for rr in (r + dr, r - dr):
            worst = max(worst, _relF(R.combine(f1, f2, rr), F))
    return worst


def _check_call(fr, p1, p2, thr, tally):
    st_d, info = fr.find(p1, p2, thr, with_info=True)
    tr = fr.trace()
    st_r, T = R.find(p1, p2, thr)
    n = len(p1)
    path = info["path"]
    assert path == T["path"]
    # (1) the sample stream, bit for bit (the device reports the whole stream; so does the reference)
    assert info["n_subsets"] == T["n_subsets"]
    np.testing.assert_array_equal(tr["subsets"], T["subsets"])
    run = min(info["iters"], info["n_subsets"])
    # (2) each candidate's score is the reference's error function on the device's own F
    for h in range(run):
        for m in range(int(tr["nmodels"][h])):
            want = R.score_candidates(path, tr["F"][h, m].ravel(), p1, p2, thr)
            assert int(tr["score"][h, m]) == want, (h, m)
    # (3) the walk replayed from the device's scores reproduces the device's walk and status
    it, bi, br, bmed = R.walk(path, n, T["niters0"], info["n_subsets"], tr["nmodels"], tr["score"], 0.99)
    assert (it, bi, br) == (info["iters"], info["best_iter"], info["best_root"])
    Fd = tr["F"][bi, br].ravel() if bi >= 0 else np.zeros(9)
    np.testing.assert_array_equal(info["F"].ravel(), Fd)
    if path == "lmeds" and bi >= 0:
        assert bmed == info["best_median"]
    np.testing.assert_array_equal(st_d, R.final_mask(path, n, Fd, bi, bmed, p1, p2, thr))
    assert info["n_inliers"] == int(st_d.sum())
    # (4) F against the reference's F over the hypotheses both solved
    f_bad = False
    both = min(run, len(T["nmodels"]))
    for h in range(both):
        idx = list(T["subsets"][h])
        if tr["nmodels"][h] != T["nmodels"][h]:
            f_bad = True
            tally["nmodels_differ"] += 1
            continue
        if tr["nmodels"][h] == 0:
            continue
        A = np.array(R.system(p1[idx], p2[idx]))
        sv = np.linalg.svd(A, compute_uv=False)
        gap = sv[6] / sv[0]
        for m in range(int(tr["nmodels"][h])):
            d = _relF(tr["F"][h, m], T["F"][h, m])
            tally["cands"] += 1
            tally["max_rel"] = max(tally["max_rel"], d if np.isfinite(d) else 0.0)
            if d == 0:
                tally["bit_equal"] += 1
            if d > F_RTOL:
                f_bad = True
                kap = _kappa(p1, p2, idx)
                if kap > KAPPA_CUT:
                    tally["ill_conditioned"] += 1
                else:
                    tally["unexplained_F"].append((n, h, m, d, kap, gap))
            else:
                tally["min_gap_ok"] = min(tally["min_gap_ok"], gap)
    # (5) the final status
    tally["calls"] += 1
    if (st_d == st_r).all():
        return
    if f_bad:
        tally["explained_F"] += 1
        return
    if R.lmeds_rounding_decided(path, n, (bi, br), (T["best_iter"], T["best_root"]), tr["score"], T["score"]):
        tally["lmeds_rounding"] += 1
        return
    diff = np.nonzero(st_d != st_r)[0]
    t = np.float32(thr * thr) if path != "lmeds" else np.float32(R.lmeds_sigma(n, T["best_median"]) ** 2)
    e = R.errors(T["F_best"], p1, p2)[diff]
    lo, hi = t, t
    for _ in range(ULP_BAND):
        lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
    if ((e >= lo) & (e <= hi)).all():
        tally["explained_ulp"] += 1
    else:
        tally["unexplained"].append((n, path, diff[:5].tolist()))


def test_device_ransac_matches_the_restatement(pkg, fr):
    tally = dict(calls=0, cands=0, bit_equal=0, max_rel=0.0, ill_conditioned=0, nmodels_differ=0, explained_F=0, explained_ulp=0,
                 lmeds_rounding=0, min_gap_ok=np.inf, unexplained=[], unexplained_F=[])
    paths = {"lmeds": 0, "ransac": 0}
    removed, small_lmeds = 0, 0
    for n, o, kind, seed in CASES:
        small_lmeds += n // 2 < R.MODEL_POINTS
        p1, p2, truth, _ = R.two_view(n, o, 0.3 if kind in ("general", "rotation", "planar") else 0.0, seed=seed * 1000 + n, kind=kind)
        _check_call(fr, p1, p2, 1.0, tally)
        st = fr.find(p1, p2, 1.0)
        paths[R.choose_path(n)] += 1
        removed += int((st == 0).sum())
    print("fmat parity:", {k: (len(v) if isinstance(v, list) else v) for k, v in tally.items()}, paths)
    assert tally["calls"] >= 400
    assert not tally["unexplained_F"], tally["unexplained_F"][:5]
    assert not tally["unexplained"], tally["unexplained"][:5]
    assert tally["explained_F"] + tally["explained_ulp"] <= 0.01 * tally["calls"], tally
    # LMeDS at n <= 13 picks its model by medians at rounding level: traced above, bounded separately
    assert tally["lmeds_rounding"] <= 0.1 * small_lmeds, (tally, small_lmeds)
    assert paths["lmeds"] >= 100 and paths["ransac"] >= 200 and removed > 0


def test_kernel_path_and_seven_exact_points(pkg, fr):
    p1, p2, _, (Rm, t) = R.two_view(7, seed=5)
    st, info = fr.find(p1, p2, 1.0, with_info=True)
    assert info["path"] == "kernel" and st.tolist() == [1] * 7 and info["best_iter"] == 0
    Ft = R.true_F(Rm, t)
    Ft = Ft / Ft[2, 2]
    tr = fr.trace()
    err = min(_relF(tr["F"][0, m], Ft) for m in range(int(tr["nmodels"][0])))
    assert err < 1e-3


def test_collinear_set_gives_no_model_and_the_switch(pkg, fr):
    k = np.arange(40)
    p1 = np.c_[50 + 8 * k, 100 + 2 * k].astype(np.float32)
    p2 = p1 + np.float32(3)
    st, info = fr.find(p1, p2, 1.0, with_info=True)
    assert info["n_subsets"] == 0 and info["best_iter"] == -1 and not st.any()
    fr.set_check_subset(0)
    try:
        st0, info0 = fr.find(p1, p2, 1.0, with_info=True)
        _, T0 = R.find(p1, p2, 1.0, check=0)
        assert info0["n_subsets"] == T0["n_subsets"] > 0
        np.testing.assert_array_equal(fr.trace()["subsets"], T0["subsets"])
    finally:
        fr.set_check_subset(1)


@pytest.mark.parametrize("max_iters", [1, 2, 1000])
def test_iteration_limits(pkg, hip, max_iters):
    """handles with room for 1, 2 and 1000 hypotheses, on LMeDS (n = 8, whose floor of 3 iterations exceeds the first two)
    and RANSAC (n = 16): only what is exact by construction — the stream, the walk replayed on the device's own counts,
    the status on the device's own F"""
    h = pkg.FundamentalRansac(hip, max_points=64, max_iters=max_iters)
    try:
        for n in (8, 16):
            p1, p2, _, _ = R.two_view(n, 0.3, 0.3, seed=500 + n)
            st, info = h.find(p1, p2, 1.0, with_info=True)
            tr = h.trace()
            path = R.choose_path(n)
            subs, niters0 = R.sample_stream(p1, p2, n, path, max_iters, 0.99)
            assert info["path"] == path and info["n_subsets"] == len(subs) == len(tr["subsets"])
            np.testing.assert_array_equal(tr["subsets"], np.array(subs, np.int32).reshape(-1, 7))
            it, bi, br, bmed = R.walk(path, n, niters0, info["n_subsets"], tr["nmodels"], tr["score"], 0.99)
            assert (it, bi, br) == (info["iters"], info["best_iter"], info["best_root"]) and it <= niters0 <= max_iters
            Fd = tr["F"][bi, br].ravel() if bi >= 0 else np.zeros(9)
            np.testing.assert_array_equal(info["F"].ravel(), Fd)
            np.testing.assert_array_equal(st, R.final_mask(path, n, Fd, bi, bmed, p1, p2, 1.0))
            assert info["n_inliers"] == int(st.sum())
    finally:
        h.close()


def test_error_paths(pkg, hip):
    h = pkg.FundamentalRansac(hip, max_points=64, max_iters=100)
    p1, p2, _, _ = R.two_view(65, seed=1)
    for n in (6, 0):
        with pytest.raises(pkg.LviError) as e:
            h.find(p1[:n], p2[:n])
        assert e.value.code == pkg._abi.LVI_ERR_INVALID_ARG
    with pytest.raises(pkg.LviError) as e:
        h.find(p1, p2)                                                 # 65 > max_points
    assert e.value.code == pkg._abi.LVI_ERR_INVALID_ARG
    st = h.find(p1[:64], p2[:64])
    assert st.shape == (64,)
    h.close()
    with pytest.raises(pkg.LviError) as e:
        h.find(p1[:20], p2[:20])                                       # destroyed handle
    assert e.value.code == pkg._abi.LVI_ERR_INVALID_ARG
    for bad in ((2, 1000), (5000, 1000), (100, 0), (100, 100000)):
        with pytest.raises(pkg.LviError):
            pkg.FundamentalRansac(hip, max_points=bad[0], max_iters=bad[1])
