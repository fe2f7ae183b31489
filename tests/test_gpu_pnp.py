"""GPU tier of the device PnP RANSAC (include/lvi_pnp.h) against the host restatement tests/pnp_ref.py, call
for call: the sample stream bit for bit, every hypothesis's inlier count against the restatement's error function on the
device's own (R, t) (exact: no transcendental lies between them), the walk replayed from the device's counts, and — on
the list whose calls tests/test_pnp_ref.py shows not to be rounding-decided — status, inlier count and iteration count
equal to pnp_ref.solve with no allowance.  The pose difference is reported, and gated only on exact geometry."""
import ctypes as C

import numpy as np
import pytest

import pnp_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pr(pkg, hip):
    h = pkg.PnPRansac(hip, max_points=2048, max_iters=100)
    yield h
    h.close()


def _check_hypotheses(h, p3, p2, max_iters, threshold=P.THRESHOLD):
    """the per-hypothesis checks of one call -> (status, info, trace)"""
    st, info = h.solve(p3, p2, threshold, with_info=True)
    tr = h.trace()
    n = len(p3)
    # (1) the sample stream, bit for bit
    want = np.array(P.sample_stream(n, max_iters), np.int32).reshape(-1, 5)
    assert info["n_subsets"] == len(want) == len(tr["subsets"])
    np.testing.assert_array_equal(tr["subsets"], want)
    assert info["path"] == ("direct" if n == 5 else "ransac")
    # (2) every hypothesis's count is the restatement's error function on the device's own (R, t)
    for k in range(info["n_subsets"]):
        if tr["has_model"][k]:
            assert int(tr["good"][k]) == int(P.inliers(tr["R"][k], tr["t"][k], p3, p2, threshold).sum()), k
        else:
            assert int(tr["good"][k]) == 0 and not tr["R"][k].any() and not tr["t"][k].any(), k
    # (3) the walk replayed from the device's counts reproduces the device's walk and status
    it, best = P.walk(n, max_iters, tr["has_model"], tr["good"])
    assert (it, best) == (info["iters"], info["best_iter"])
    if best < 0:
        want_st = np.zeros(n, np.uint8)
        assert not info["R"].any() and not info["t"].any() and info["which_beta"] == 0
    else:
        want_st = np.ones(n, np.uint8) if n == 5 else P.inliers(tr["R"][best], tr["t"][best], p3, p2, threshold)
        np.testing.assert_array_equal(info["R"], tr["R"][best])
        np.testing.assert_array_equal(info["t"], tr["t"][best])
        assert info["which_beta"] in (1, 2, 3)
    np.testing.assert_array_equal(st, want_st)
    assert info["n_inliers"] == int(st.sum())
    return st, info, tr


def _compare_poses(tr, T, tally, which):
    for k in which:
        m = T["models"][k]
        if m is None or not tr["has_model"][k]:
            assert m is None and not tr["has_model"][k], k
            continue
        d = max(np.abs(tr["R"][k] - m["R"]).max(), np.abs(tr["t"][k] - m["t"]).max())
        tally["hyp"] += 1
        tally["bit_equal"] += int(tr["R"][k].tobytes() == m["R"].tobytes() and tr["t"][k].tobytes() == m["t"].tobytes())
        if np.isfinite(d):
            tally["max_diff"] = max(tally["max_diff"], float(d))


def test_device_pnp_matches_the_restatement(pr):
    cases = P.gpu_cases()
    assert 120 <= len(cases) <= 144
    tally = dict(calls=0, hyp=0, bit_equal=0, max_diff=0.0, chosen=0, chosen_max_diff=0.0, exact_calls=0)
    chosen = dict(hyp=0, bit_equal=0, max_diff=0.0)
    for n, o, noise, seed in cases:
        p3, p2, truth, (Rt, tt) = P.scene(n, o, noise, seed)
        st, info, tr = _check_hypotheses(pr, p3, p2, 100)
        st_r, T = P.solve(p3, p2)
        # the final status: exactly the restatement's, no allowance
        np.testing.assert_array_equal(st, st_r, err_msg=str((n, o, noise, seed)))
        assert (info["n_inliers"], info["iters"], info["best_iter"]) == (T["n_inliers"], T["iters"], T["best_iter"]), (n, o, noise, seed)
        # pose differences: every hypothesis the restatement solved, and those chosen by either walk
        _compare_poses(tr, T, tally, range(T["iters"]))
        _compare_poses(tr, T, chosen, sorted({b for b in (info["best_iter"], T["best_iter"]) if 0 <= b < T["iters"]}))
        b = info["best_iter"]
        if noise == 0 and b >= 0 and truth[tr["subsets"][b]].all():
            # exact geometry: the chosen pose is the scene's, within 10 x the bound measured with LAPACK (pnp_ref.EXACT_*)
            assert np.abs(tr["R"][b] - Rt).max() <= 10 * P.EXACT_DR and np.abs(tr["t"][b] - tt).max() <= 10 * P.EXACT_DT, (n, o, seed)
            assert st[truth].all() and not st[~truth].any()
            tally["exact_calls"] += 1
        tally["calls"] += 1
    tally["chosen"], tally["chosen_max_diff"] = chosen["hyp"], chosen["max_diff"]
    print("pnp parity:", tally, "chosen bit-equal:", chosen["bit_equal"])
    assert tally["calls"] == len(cases) and tally["hyp"] > 1000 and tally["exact_calls"] >= 40


@pytest.mark.parametrize("max_iters", [1, 1024])
def test_iteration_limits(pkg, hip, max_iters):
    h = pkg.PnPRansac(hip, max_points=256, max_iters=max_iters)
    try:
        p3, p2, truth, _ = P.scene(150, 0.4, 0.5 / P.FOCAL_LENGTH, 77)
        st, info, tr = _check_hypotheses(h, p3, p2, max_iters)
        st_r, T = P.solve(p3, p2, max_iters=max_iters)
        np.testing.assert_array_equal(st, st_r)
        assert (info["iters"], info["best_iter"], info["n_subsets"]) == (T["iters"], T["best_iter"], max_iters)
        if max_iters == 1:
            assert info["iters"] == 1
    finally:
        h.close()


@pytest.mark.parametrize("kind", ["planar", "identical", "outliers_0.6"])
def test_calls_outside_the_status_contract(pr, kind):
    """degenerate geometry and an outlier share at which half of the calls find no model: only the per-hypothesis checks
    and that the call returns"""
    if kind == "outliers_0.6":
        p3, p2, _, _ = P.scene(150, 0.6, 1.0 / P.FOCAL_LENGTH, 5)
    else:
        p3, p2, _, _ = P.scene(40, 0.0, 0.0, 6, kind=kind)
    st, info, tr = _check_hypotheses(pr, p3, p2, 100)
    assert st.shape == (len(p3),)
    if kind == "planar":                                              # z = 8 exactly: every control-point matrix is exactly singular
        assert not tr["has_model"].any() and info["best_iter"] == -1 and info["iters"] == 100 and not st.any()


def test_error_paths_write_nothing(pkg, hip):
    pkg.pnp.bind(hip)
    dll, INV = hip.dll, pkg._abi.LVI_ERR_INVALID_ARG
    assert dll.lvi_pnp_abi_version() == 1 and dll.lvi_abi_version() == 6
    h = pkg.PnPRansac(hip, max_points=64, max_iters=100)
    p3, p2, _, _ = P.scene(65, seed=1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for n, status_ok in ((4, True), (0, True), (65, True), (30, False)):
        st = np.full(80, 7, np.uint8)
        info = pkg.pnp.PnPInfo()
        info.path = info.iters = info.best_iter = 7
        assert dll.lvi_pnp_solve(h._h, vp(p3), vp(p2), n, P.THRESHOLD, 0.99, vp(st) if status_ok else None, C.byref(info)) == INV
        assert (st == 7).all() and (info.path, info.iters, info.best_iter) == (7, 7, 7)
    for n in (4, 65):
        with pytest.raises(pkg.LviError) as e:
            h.solve(p3[:n], p2[:n])
        assert e.value.code == INV
    assert h.solve(p3[:64], p2[:64]).shape == (64,)
    h.close()
    with pytest.raises(pkg.LviError) as e:
        h.solve(p3[:20], p2[:20])                                      # destroyed handle
    assert e.value.code == INV
    for bad in ((4, 100), (2049, 100), (100, 0), (100, 1025)):
        with pytest.raises(pkg.LviError):
            pkg.PnPRansac(hip, max_points=bad[0], max_iters=bad[1])
