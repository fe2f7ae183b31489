"""GPU tier of the GPS factors and the marginal covariance of the pose graph (include/lvi_pgo_gps.h) against the
float64 reference tests/pgo_gps_ref.py.

Comparison.  GPS fixes the gauge, so the device's poses are compared with the reference's ABSOLUTELY, every key, as
rotation angle and translation.  The tolerance per scene is max(10 G, 10 conv_eps), G the distance between the reference's
two linear solvers on that scene (the convention of test_gpu_pgo.py); chi2_after by the rule of its _check.  A covariance
is compared relative to max|C| within max(10 G_cov, 1e-9), G_cov the gap between the reference's two routes at the poses
the DEVICE holds (the reference graph takes them over, so both sides linearise at the same point).  Every figure is
printed before it is asserted; DESIGN §19 records them."""
import numpy as np
import pytest

import pgo_gps_ref as GR
import pgo_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
FLOOR = 10 * R.CONV_EPS
CHI2_ZERO = 1e-20                  # as in test_gpu_pgo.py
COV_FLOOR = 1e-9
INVALID_ARG, CAPACITY, STATE = -1, -4, -5


@pytest.fixture(scope="module")
def refs():
    """(scene, full_logmap) -> (scene dict, lstsq poses, lstsq info, chol poses, chol info), computed once and never changed"""
    cache = {}

    def get(name, full):
        if (name, full) not in cache:
            sc = GR.gps_scene(name)
            (Xa, ia), (Xb, ib) = GR.solve_both(GR.build(sc, GR.GpsGraph(full, max_iters=GR.GPS_MAX_ITERS)))
            cache[(name, full)] = (sc, Xa, ia, Xb, ib)
        return cache[(name, full)]
    return get


def _device_graph(pkg, hip, sc, full, **kw):
    n, nl = len(sc["poses"]), len(sc["loops"])
    return GR.build(sc, pkg.PoseGraph(hip, max_poses=n, max_loops=max(nl, 1), full_logmap=full, **kw))


def _check_minimiser(tag, Xd, info, Xa, ia, Xb, ib):
    gr, gt = GR.abs_gaps(Xa, Xb)
    dr, dt = GR.abs_gaps(Xa, Xd)
    tol = [max(10 * g, FLOOR) for g in (gr, gt)]
    gchi = abs(ia["chi2_after"] - ib["chi2_after"]) / max(ia["chi2_after"], 1e-300) if ia["chi2_after"] > 0 else 0.0
    mchi = max(10 * gchi, FLOOR)
    dchi = abs(info["chi2_after"] - ia["chi2_after"])
    print(f"[pgo gps] {tag}: G absolute (rad, m) = ({gr:.3e}, {gt:.3e}); device absolute = ({dr:.3e}, {dt:.3e}); tolerances {['%.3e' % t for t in tol]}; "
          f"iterations device {info['iterations']} reference {ia['iterations']} / {ib['iterations']}; max_step {info['max_step']:.3e}; "
          f"chi2 {info['chi2_before']:.9g} -> {info['chi2_after']:.12g} (reference {ia['chi2_before']:.9g} -> {ia['chi2_after']:.12g}, |diff| {dchi:.3e}, "
          f"margin {mchi:.3e} relative)")
    assert ia["converged"] and ib["converged"], tag
    assert info["converged"] and info["status"] == 0 and info["max_step"] < R.CONV_EPS, tag
    assert info["chi2_after"] < info["chi2_before"], tag
    assert dr <= tol[0] and dt <= tol[1], tag
    assert dchi <= mchi * ia["chi2_after"] + CHI2_ZERO, tag
    assert abs(info["chi2_before"] - ia["chi2_before"]) <= 1e-9 * ia["chi2_before"] + CHI2_ZERO, tag


def _check_cov(tag, C, Ca, Cb):
    """device C against the reference's two routes Ca, Cb -> the tolerance used"""
    gcov = GR.cov_gap(Ca, Cb)
    tol = max(10 * gcov, COV_FLOOR)
    scale = np.abs(Ca).max()
    dev = float(np.abs(C - Ca).max() / scale)
    asym = float(np.abs(C - C.T).max() / scale)
    print(f"[pgo gps] covariance {tag}: G_cov {gcov:.3e}, tolerance {tol:.3e}, device {dev:.3e}, asymmetry {asym:.3e} (all relative to max|C| = {scale:.6g}); "
          f"(3,3) {C[3, 3]:.9g}, (4,4) {C[4, 4]:.9g}")
    assert np.isfinite(C).all(), tag
    assert dev <= tol and asym <= tol, tag
    assert (np.diag(C) > 0).all(), tag
    return tol


def _reference_at(sc, full, T):
    """the reference graph of a scene at the poses T"""
    g = GR.build(sc, GR.GpsGraph(full))
    g.X = [np.array(t, F64) for t in T]
    return g


# ---- the minimiser ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [1, 0])
@pytest.mark.parametrize("name", list(GR.GPS_SCENES))
def test_pgo_gps_minimiser_and_covariance(pkg, hip, refs, name, full):
    """every scene with both charts: the device's minimiser against the reference's, absolutely and for every key; then the
    marginal covariance of the last key at the poses the device holds"""
    sc, Xa, ia, Xb, ib = refs(name, full)
    n = len(sc["poses"])
    g = _device_graph(pkg, hip, sc, full, max_iters=GR.GPS_MAX_ITERS)
    assert g.count() == (n, len(sc["loops"])) and g.gps_count() == len(sc["gps"])
    info = g.solve()
    T, p = g.poses()
    C = g.marginal_covariance(n - 1)
    T2, p2 = g.poses()
    g.close()
    _check_minimiser(f"{name} full_logmap {full}", T, info, Xa, ia, Xb, ib)
    np.testing.assert_array_equal(p.view(np.uint32), np.array([R.pose_to_rpyxyz(t) for t in T], F32).view(np.uint32))
    for t in T:
        assert np.abs(t[:3, :3] @ t[:3, :3].T - np.eye(3)).max() < 1e-12
    assert info["iterations"] >= 2
    # the covariance call took no step
    np.testing.assert_array_equal(T2, T)
    np.testing.assert_array_equal(p2.view(np.uint32), p.view(np.uint32))
    ref = _reference_at(sc, full, T)
    Ca, Cb = ref.marginal_covariance(n - 1, "qr"), ref.marginal_covariance(n - 1, "chol")
    _check_cov(f"{name} full_logmap {full}, key {n - 1}", C, Ca, Cb)
    if name == "g20_mid":
        # a fix exists and the gate of mapOptimization.cpp:1443 stays open all the same: weak yaw about the fix x lever arm
        assert C[3, 3] > 25.0 and Ca[3, 3] > 25.0


def test_pgo_gps_default_max_iters_stops_and_a_second_solve_finishes(pkg, hip, refs):
    """g64 needs more undamped steps than the default max_iters 10: the first call stops with the soft status, a second one
    finishes, and the answer is the reference's"""
    sc, Xa, ia, Xb, ib = refs("g64", 1)
    assert ia["iterations"] > R.MAX_ITERS + 1 and ia["steps"][R.MAX_ITERS - 1] > 10 * R.CONV_EPS
    g = _device_graph(pkg, hip, sc, 1)
    assert g.params.max_iters == R.MAX_ITERS
    first = g.solve()
    print(f"[pgo gps] g64, default max_iters: status {first['status']}, iterations {first['iterations']}, max_step {first['max_step']:.3e}")
    assert first["status"] == pkg.pgo.NOT_CONVERGED and not first["converged"] and first["iterations"] == R.MAX_ITERS
    second = g.solve()
    T, _ = g.poses()
    g.close()
    assert first["iterations"] + second["iterations"] >= ia["iterations"] - 1
    second = dict(second, chi2_before=first["chi2_before"])
    _check_minimiser("g64 in two solves", T, second, Xa, ia, Xb, ib)


# ---- the covariance ----------------------------------------------------------------------------------------
def test_pgo_covariance_of_one_key_is_its_prior(pkg, hip):
    """the known answer: one key at its prior -> diag(1e-2, 1e-2, pi^2, 1e8, 1e8, 1e8) (mapOptimization.cpp:1418-1420)"""
    for full in (1, 0):
        g = pkg.PoseGraph(hip, max_poses=4, max_loops=1, full_logmap=full)
        g.add_pose(None, F32([0.1, -0.2, 2.5, 30.0, -12.0, 1.5]))
        C = g.marginal_covariance(0)
        g.close()
        want = np.diag(R.PRIOR_VAR)
        gap = np.abs(C - want).max() / 1e8
        print(f"[pgo gps] covariance of one key, full_logmap {full}: |C - prior| / 1e8 = {gap:.3e}; diagonal {np.diag(C)}")
        assert gap <= COV_FLOOR
        assert np.abs(np.diag(C) / R.PRIOR_VAR - 1).max() <= 1e-9            # each entry, relative to itself


@pytest.mark.parametrize("full", [1, 0])
def test_pgo_covariance_without_gps_is_the_gauge_split(pkg, hip, full):
    """n37 after its solve, keys 0, 17 and 36: the closed-form gauge part plus the block of the anchored system, against a QR
    factorisation of the whitened Jacobian and the reference's own split"""
    sc = R.gpu_scene("n37")
    g = R.build(sc, pkg.PoseGraph(hip, max_poses=37, max_loops=3, full_logmap=full))
    assert g.gps_count() == 0
    g.solve()
    T, _ = g.poses()
    ref = _reference_at(sc, full, T)
    for key in (0, 17, 36):
        C = g.marginal_covariance(key)
        _check_cov(f"n37 without GPS, full_logmap {full}, key {key}", C, ref.marginal_covariance(key, "qr"), ref.marginal_covariance(key, "split"))
    np.testing.assert_array_equal(g.poses()[0], T)
    g.close()


# ---- a graph without GPS factors is what it was ------------------------------------------------------------------
def test_pgo_cleared_of_gps_equals_a_fresh_handle(pkg, hip):
    sc = GR.gps_scene("g37_key0")
    plain = dict(sc, gps=[])
    g = _device_graph(pkg, hip, sc, 1, max_iters=GR.GPS_MAX_ITERS)
    with_gps = g.solve()
    Tg, _ = g.poses()
    g.clear()
    assert g.count() == (0, 0) and g.gps_count() == 0
    g.set_params(max_iters=R.MAX_ITERS)
    GR.build(plain, g)
    fresh = _device_graph(pkg, hip, plain, 1)
    ia, ib = g.solve(), fresh.solve()
    (Ta, pa), (Tb, pb) = g.poses(), fresh.poses()
    Ca, Cb = g.marginal_covariance(36), fresh.marginal_covariance(36)
    g.close(); fresh.close()
    assert ia == ib and ia["converged"]
    np.testing.assert_array_equal(Ta, Tb)
    np.testing.assert_array_equal(pa.view(np.uint32), pb.view(np.uint32))
    np.testing.assert_array_equal(Ca, Cb)
    assert with_gps["converged"] and np.abs(Tg - Ta).max() > 1e-3             # the GPS factor had moved the graph


# ---- errors -------------------------------------------------------------------------------------------------
def test_pgo_gps_argument_and_capacity_errors(pkg, hip):
    """every refused call leaves the graph as it was: the answer equals a twin's that never saw the refused calls"""
    sc = GR.gps_scene("g5")
    g = pkg.PoseGraph(hip, max_poses=5, max_loops=1, max_iters=GR.GPS_MAX_ITERS)
    z, v = F32([1, 2, 3]), F32([1, 2, 1])
    with pytest.raises(pkg.LviError) as e:
        g.marginal_covariance(0)
    assert e.value.code == STATE                                          # no poses
    with pytest.raises(pkg.LviError) as e:
        g.add_gps(0, z, v)
    assert e.value.code == INVALID_ARG                                    # no keys yet
    R.build(sc, g)
    twin = _device_graph(pkg, hip, sc, 1, max_iters=GR.GPS_MAX_ITERS)
    key, xyz, var = sc["gps"][0]
    g.add_gps(key, xyz, var)
    nan, inf = float("nan"), float("inf")
    bad = [(-1, z, v), (5, z, v), (2, z, F32([0, 1, 1])), (2, z, F32([1, -1, 1])), (2, z, F32([1, 1, nan])), (2, z, F32([inf, 1, 1])),
           (2, F32([nan, 0, 0]), v), (2, F32([0, inf, 0]), v), (2, F32([0, 0, -inf]), v)]
    for k, zz, vv in bad:
        with pytest.raises(pkg.LviError) as e:
            g.add_gps(k, zz, vv)
        assert e.value.code == INVALID_ARG, (k, zz, vv)
        assert g.gps_count() == 1 and g.count() == (5, 0)
    for k in (-1, 5):
        with pytest.raises(pkg.LviError) as e:
            g.marginal_covariance(k)
        assert e.value.code == INVALID_ARG
    ia, ib = g.solve(), twin.solve()
    assert ia == ib and ia["converged"]
    np.testing.assert_array_equal(g.poses()[0], twin.poses()[0])
    np.testing.assert_array_equal(g.marginal_covariance(4), twin.marginal_covariance(4))
    # capacity: max_poses factors in total
    for _ in range(4):
        g.add_gps(key, xyz, var)
    assert g.gps_count() == 5
    with pytest.raises(pkg.LviError) as e:
        g.add_gps(key, xyz, var)
    assert e.value.code == CAPACITY and g.gps_count() == 5
    g.clear()
    assert g.gps_count() == 0
    g.close(); twin.close()


# ---- node level ------------------------------------------------------------------------------------------
SEQ_P = dict(N_SCAN=4, Horizon_SCAN=8192, max_raw_points=20000, max_map_points=600000, max_keyframes=64, max_keyframe_points=600000)
FIX_OFFSET, FIX_COV = np.array([0.2, -0.1, 0.7]), (0.5, 0.5, 0.5)


def _rows_to_rpyxyz(rows):
    """lvh_seq_keyposes rows (x y z roll pitch yaw time index) -> (roll, pitch, yaw, x, y, z) float32"""
    return np.ascontiguousarray(rows[:, [3, 4, 5, 0, 1, 2]], F32)


def _dist32(a, b):
    d = F32(a) - F32(b)
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def test_pgo_node_takes_gps_fixes_through_the_covariance_gate(pkg, hip, oracle):
    """the revisit_a replay of test_gpu_pgo.py's node test with useGps and one synthetic fix per key (0.5 variance, the key's
    position moved by FIX_OFFSET).  addGPSFactor's decisions are predicted here from the node's own stored covariance; the
    graph the node built is then rebuilt in the reference from what the node handed over, and minimised"""
    import loop_scenes as SC
    H = pkg.host_api
    sc = SC.scene("revisit_a", SC.base_passes(pkg, oracle))
    kfs, stamps = sc["kfs"], sc["stamps"]
    n = SC.CUR + 1
    want = np.array([k[2] for k in kfs], F32)
    fixes = [np.array(k[2][3:], F64) + FIX_OFFSET for k in kfs]
    runs = {}
    for mode in ("plain", "ignored", "gps"):
        m = H.SequentialMapper(pkg.load_host(), hip, pkg.default_params(hip, **SEQ_P), incremental_map=1)
        pg = H.PoseGraphBackend(pkg.load_host(), hip, max_poses=64, max_loops=8, max_iters=GR.GPS_MAX_ITERS)
        m.usePoseGraph(pg)
        if mode == "gps":
            m.useGps(use_gps_elevation=False, gps_cov_threshold=2.0, pose_cov_threshold=25.0)      # utility.h:178-183
        lc = H.LoopCloser(pkg.load_host(), m, search_radius=15.0, search_time_diff=30.0, search_num=SC.SEARCH, fitness_score=SC.FITNESS_GATE, surf_leaf=SC.LEAF)
        lc.reserve(1 << 16, 1 << 20)
        log, c = [], None
        for k in range(n + 1):
            if k == n:                                                    # the loop constraint, as in test_gpu_pgo.py
                pushed, _ = lc.performLoopClosure(stamps[n - 1])
                assert pushed
                c = lc.pop()
                assert pg.push_loop(c) == 1
            if mode != "plain":
                m.gpsHandler(stamps[k], fixes[k], FIX_COV)
            before = m.keyposes()
            m.seed_keyframe(kfs[k][0], kfs[k][1], kfs[k][2], stamps[k])
            last = m.gps_last()
            log.append(dict(pose_from=_rows_to_rpyxyz(before)[-1] if k else None, cov=last["pose_covariance"].copy(), added=last["factors_added"],
                            lib_cov=pg.graph.marginal_covariance(k) if mode == "gps" else None, corrected=m.poses_corrected(), queued=last["queued"],
                            updates=pg.last()["updates"]))
        runs[mode] = dict(log=log, c=c, after=m.keyposes(), graph=pg.graph.poses(), count=pg.graph.count(), gps=pg.graph.gps_count(), last=pg.last(),
                          in_use=m.gps_last()["in_use"])
        lc.close()
        m.usePoseGraph(None)
        m.close()
        pg.close()
    a, b, g = runs["plain"], runs["ignored"], runs["gps"]
    # without useGps the messages only queue up: every answer is the run's that never saw one
    assert not a["in_use"] and not b["in_use"] and g["in_use"]
    assert a["gps"] == b["gps"] == 0 and a["count"] == b["count"] == (n + 1, 1)
    assert [e["queued"] for e in b["log"]] == list(range(1, n + 2)) and all(e["added"] == 0 and not e["cov"].any() for e in a["log"] + b["log"])
    np.testing.assert_array_equal(a["after"], b["after"])
    np.testing.assert_array_equal(a["graph"][0], b["graph"][0])
    np.testing.assert_array_equal(a["c"]["between"], b["c"]["between"])
    assert {k: v for k, v in a["last"].items() if k != "pose_to"} == {k: v for k, v in b["last"].items() if k != "pose_to"}
    assert [e["corrected"] for e in a["log"]] == [e["corrected"] for e in b["log"]] == [0] * n + [1]
    for e, p in zip(a["log"][1:], want[:-1]):                             # the odometry chain until the loop is applied
        np.testing.assert_array_equal(e["pose_from"].view(np.uint32), p.view(np.uint32))
    # with useGps: addGPSFactor's decisions, predicted from the covariance the node stored after the key before
    log = g["log"]
    lastfix, added, expect, accepted = np.zeros(3, F32), 0, [], []
    front = want[0][3:]
    for k in range(n + 1):
        took = False
        if k >= 1:
            back = log[k]["pose_from"][3:]                                # cloudKeyPoses3D.back() before the new key is pushed
            cov = log[k - 1]["cov"]
            gate_open = not (cov[3, 3] < 25.0 and cov[4, 4] < 25.0)
            cur = F32([fixes[k][0], fixes[k][1], want[k][5]])             # without useGpsElevation z is transformTobeMapped[5]
            if not _dist32(front, back) < 5.0 and gate_open and not _dist32(cur, lastfix) < 5.0:
                took, lastfix = True, cur
                accepted.append((k, cur))
        added += took
        expect.append(added)
    got = [e["added"] for e in log]
    print(f"[pgo gps] node: GPS factors after each key {got}; predicted {expect}; (3,3), (4,4) after each key "
          f"{[(round(float(e['cov'][3, 3]), 3), round(float(e['cov'][4, 4]), 3)) for e in log]}")
    assert got == expect and g["gps"] == added == len(accepted)
    first = accepted[0][0]
    # the first fix is taken as soon as the path exceeds 5 m: the prior's 1e8 has kept the gate open since key 0
    assert first == min(k for k in range(1, n + 1) if not _dist32(front, want[k - 1][3:]) < 5.0) and log[0]["cov"][3, 3] > 1e7
    assert all(e["cov"][3, 3] > 25.0 for e in log[:first]) and log[first]["cov"][3, 3] < 25.0 and log[first]["cov"][4, 4] < 25.0
    refused = [k for k in range(first + 1, n + 1) if log[k - 1]["cov"][3, 3] < 25.0 and log[k - 1]["cov"][4, 4] < 25.0]
    assert refused and all(got[k] == got[k - 1] for k in refused)          # later fixes are refused while both entries are below 25
    # the stored covariance is the library's for the newest key, after every key
    for k, e in enumerate(log):
        np.testing.assert_array_equal(e["cov"], e["lib_cov"], err_msg=f"key {k}")
    # a solve and a correction per accepted fix, and one for the loop (unless its key took a fix too)
    solves = sorted(set([k for k, _ in accepted] + [n]))
    assert [e["updates"] for e in log] == [sum(1 for s in solves if s <= k) for k in range(n + 1)]
    assert [e["corrected"] for e in log] == [e["updates"] for e in log]
    assert g["last"]["status"] == 0 and g["last"]["converged"] and g["count"] == (n + 1, 1)
    # the key poses after correctPoses are the float casts of the graph's doubles
    T, p = g["graph"]
    np.testing.assert_array_equal(_rows_to_rpyxyz(g["after"]).view(np.uint32), p.view(np.uint32))
    np.testing.assert_array_equal(p.view(np.uint32), np.array([R.pose_to_rpyxyz(t) for t in T], F32).view(np.uint32))
    # the reference minimiser of the graph the node built: the float poses it handed to addOdomFactor, the fixes it took, the loop
    ref = GR.GpsGraph(1, max_iters=GR.GPS_MAX_ITERS)
    for k in range(n + 1):
        ref.add_pose(log[k]["pose_from"], want[k])
    for k, cur in accepted:
        ref.add_gps(k, cur, F32([1, 1, 1]))                               # max(0.5, 1.0f) twice and max(0.01f, 1.0f)
    ref.add_loop(g["c"]["key_cur"], g["c"]["key_pre"], g["c"]["between"], g["c"]["noise"])
    (Xa, ia), (Xb, ib) = GR.solve_both(ref)
    gr, gt = GR.abs_gaps(Xa, Xb)
    dr, dt = GR.abs_gaps(Xa, T)
    tol = [max(10 * x, FLOOR) for x in (gr, gt)]
    print(f"[pgo gps] node: fixes on keys {[k for k, _ in accepted]}; G absolute ({gr:.3e}, {gt:.3e}), device absolute ({dr:.3e}, {dt:.3e}), tolerances "
          f"{['%.3e' % t for t in tol]}; chi2_after device {g['last']['chi2_after']:.12g} reference {ia['chi2_after']:.12g}")
    assert ia["converged"] and ib["converged"] and dr <= tol[0] and dt <= tol[1]
    mchi = max(10 * abs(ia["chi2_after"] - ib["chi2_after"]) / ia["chi2_after"], FLOOR)
    assert abs(g["last"]["chi2_after"] - ia["chi2_after"]) <= mchi * ia["chi2_after"] + CHI2_ZERO
    moved = np.abs(_rows_to_rpyxyz(g["after"])[:, 3:] - _rows_to_rpyxyz(a["after"])[:, 3:]).max()
    print(f"[pgo gps] node: the fixes moved the key poses by up to {moved:.4f} m against the run without GPS")
    assert moved > 0.05                                                   # FIX_OFFSET is 0.2 m in x: far above the float resolution of a pose here
