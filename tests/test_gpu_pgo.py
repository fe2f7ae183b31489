"""GPU tier of the pose-graph optimiser (include/lvi_pgo.h) against its float64 reference tests/pgo_ref.py.

Comparison.  The poses relative to key 0 (X0^-1 Xi: rotation angle and translation) and key 0 itself are compared apart.
For each group the tolerance is 10 x the gap G between the reference's two linear solvers on that scene, computed here,
and never below 10 x conv_eps, which is how close two converged runs are guaranteed to be.  chi2_after must lie within the
same relative margin of the reference minimum.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import pgo_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
FLOOR = 10 * R.CONV_EPS
# two sums of squares of whitened rounding residues (1e3 x 1e-16 per component) differ by this at most when the minimum is zero
CHI2_ZERO = 1e-20


@pytest.fixture(scope="module")
def refs():
    """(scene name, full_logmap) -> (scene, lstsq poses, lstsq info, chol poses, chol info), computed once and never changed"""
    cache = {}

    def get(name, full):
        if (name, full) not in cache:
            sc = R.gpu_scene(name)
            (Xa, ia), (Xb, ib) = R.solve_both(R.build(sc, R.Graph(full)))
            cache[(name, full)] = (sc, Xa, ia, Xb, ib)
        return cache[(name, full)]
    return get


def _check(tag, Xd, info, Xa, ia, Xb, ib):
    (gr, gt), (g0r, g0t) = R.gaps(Xa, Xb)
    (dr, dt), (d0r, d0t) = R.gaps(Xa, Xd)
    tol = [max(10 * g, FLOOR) for g in (gr, gt, g0r, g0t)]
    gchi = abs(ia["chi2_after"] - ib["chi2_after"]) / max(ia["chi2_after"], 1e-300) if ia["chi2_after"] > 0 else 0.0
    mchi = max(10 * gchi, FLOOR)
    dchi = abs(info["chi2_after"] - ia["chi2_after"])
    print(f"[pgo] {tag}: G relative (rad, m) = ({gr:.3e}, {gt:.3e}), G key 0 = ({g0r:.3e}, {g0t:.3e}); device relative = ({dr:.3e}, {dt:.3e}), "
          f"device key 0 = ({d0r:.3e}, {d0t:.3e}); tolerances {['%.3e' % t for t in tol]}; iterations device {info['iterations']} "
          f"reference {ia['iterations']} / {ib['iterations']}; max_step {info['max_step']:.3e}; chi2 {info['chi2_before']:.9g} -> {info['chi2_after']:.12g} "
          f"(reference {ia['chi2_before']:.9g} -> {ia['chi2_after']:.12g}, |diff| {dchi:.3e}, margin {mchi:.3e} relative)")
    assert ia["converged"] and ib["converged"], tag
    assert info["converged"] and info["status"] == 0 and info["max_step"] < R.CONV_EPS, tag
    assert dr <= tol[0] and dt <= tol[1], tag
    assert d0r <= tol[2] and d0t <= tol[3], tag
    assert dchi <= mchi * ia["chi2_after"] + CHI2_ZERO, tag
    assert abs(info["chi2_before"] - ia["chi2_before"]) <= 1e-9 * ia["chi2_before"] + CHI2_ZERO, tag


def _rpy_of(T):
    return np.array([R.pose_to_rpyxyz(t) for t in T], F32)


@pytest.mark.parametrize("full", [1, 0])
@pytest.mark.parametrize("name", list(R.GPU_SCENES))
def test_pgo_minimiser(pkg, hip, refs, name, full):
    """every scene with both charts: the device's minimiser against the reference's, and the float poses"""
    sc, Xa, ia, Xb, ib = refs(name, full)
    n, nl = len(sc["poses"]), len(sc["loops"])
    g = R.build(sc, pkg.PoseGraph(hip, max_poses=n, max_loops=max(nl, 1), full_logmap=full))
    assert g.count() == (n, nl)
    T0, p0 = g.poses()
    np.testing.assert_array_equal(p0.view(np.uint32), _rpy_of(T0).view(np.uint32))
    assert np.abs(T0 - np.array([R.pose_from_rpyxyz(q) for q in sc["poses"]])).max() < 1e-15      # the initial estimate is the pose handed in
    info = g.solve()
    T, p = g.poses()
    g.close()
    _check(f"{name} full_logmap {full}", T, info, Xa, ia, Xb, ib)
    # the float poses are the f32 casts of the returned doubles
    np.testing.assert_array_equal(p.view(np.uint32), _rpy_of(T).view(np.uint32))
    assert np.abs(T[:, 3, :] - [0, 0, 0, 1]).max() == 0
    for t in T:
        assert np.abs(t[:3, :3] @ t[:3, :3].T - np.eye(3)).max() < 1e-12
    if nl == 0:
        # a chain without loops is a fixed point: one step of rounding size, the poses where they were
        assert info["iterations"] == 1 and info["max_step"] < 1e-12
        assert np.abs(T - T0).max() < 1e-12
    else:
        assert info["chi2_after"] < info["chi2_before"] and 2 <= info["iterations"] <= R.MAX_ITERS - 2


def test_pgo_windows_and_second_solve(pkg, hip, refs):
    """a window of get_poses is that slice of the whole; a second solve of a solved graph takes one step and moves nothing"""
    sc, Xa, ia, _, _ = refs("n37", 1)
    g = R.build(sc, pkg.PoseGraph(hip, max_poses=64, max_loops=8))
    g.solve()
    T, p = g.poses()
    Tw, pw = g.poses(5, 20)
    np.testing.assert_array_equal(Tw, T[5:25])
    np.testing.assert_array_equal(pw.view(np.uint32), p[5:25].view(np.uint32))
    again = g.solve()
    T2, _ = g.poses()
    print(f"[pgo] second solve: iterations {again['iterations']}, max_step {again['max_step']:.3e}, moved {np.abs(T2 - T).max():.3e}")
    assert again["converged"] and again["iterations"] == 1 and np.abs(T2 - T).max() < FLOOR
    assert abs(again["chi2_before"] - again["chi2_after"]) <= 1e-9 * again["chi2_after"]
    g.close()


def test_pgo_incremental(pkg, hip):
    """solve, add keys whose odometry edges are measured from the corrected poses, add a loop, solve again — and the
    reference doing the same with the same float poses"""
    sc = R.gpu_scene("n37")
    P0 = sc["poses"]
    n1 = 30
    dev = pkg.PoseGraph(hip, max_poses=64, max_loops=8)
    ref = R.Graph(1)
    for g in (dev, ref):
        for k in range(n1):
            g.add_pose(None if k == 0 else P0[k - 1], P0[k])
        g.add_loop(29, 0, R.pose_inv(sc["gt"][29]) @ sc["gt"][0], 0.2)
    i1 = dev.solve()
    refc = ref.copy()
    ra, rb = ref.solve("lstsq"), refc.solve("chol")
    T1, p1 = dev.poses()
    _check("incremental, first solve", T1, i1, ref.poses(), ra, refc.poses(), rb)
    # the node's next keys: pose_from = the corrected newest key pose (float), pose_to = that pose moved by the odometry increment
    cur = p1[n1 - 1].copy()
    for k in range(n1, len(P0)):
        inc = R.pose_inv(R.pose_from_rpyxyz(P0[k - 1])) @ R.pose_from_rpyxyz(P0[k])
        nxt = R.pose_to_rpyxyz(R.pose_from_rpyxyz(cur) @ inc)
        for g in (dev, ref, refc):
            g.add_pose(cur, nxt)
        cur = nxt
    Z = R.pose_inv(sc["gt"][36]) @ sc["gt"][3]
    for g in (dev, ref, refc):
        g.add_loop(36, 3, Z, 0.1)
    assert dev.count() == (37, 2)
    i2 = dev.solve()
    ra, rb = ref.solve("lstsq"), refc.solve("chol")
    T2, p2 = dev.poses()
    dev.close()
    _check("incremental, second solve", T2, i2, ref.poses(), ra, refc.poses(), rb)
    assert i2["iterations"] >= 2 and np.abs(T2[:n1] - T1).max() > 1e-6   # the second loop moved the solved keys again


def test_pgo_capacity_and_argument_errors(pkg, hip):
    """every refused call leaves the graph as it was: the answer equals a twin's that never saw the refused calls"""
    sc = R.gpu_scene("n37")
    twin = R.build(sc, pkg.PoseGraph(hip, max_poses=37, max_loops=3))
    g = pkg.PoseGraph(hip, max_poses=37, max_loops=3)
    with pytest.raises(pkg.LviError) as e:
        g.solve()
    assert e.value.code == -5                                          # no poses
    with pytest.raises(pkg.LviError) as e:
        g.add_loop(0, 1, np.eye(4), 0.1)
    assert e.value.code == -1                                          # no keys yet
    R.build(dict(poses=sc["poses"], loops=[]), g)
    Z = sc["loops"][0][2]
    for frm, to, var in ((5, 5, 0.1), (-1, 3, 0.1), (3, 37, 0.1), (37, 3, 0.1), (3, 4, 0.0), (3, 4, -1.0), (3, 4, float("nan")), (3, 4, float("inf"))):
        with pytest.raises(pkg.LviError) as e:
            g.add_loop(frm, to, Z, var)
        assert e.value.code == -1, (frm, to, var)
    bad = np.eye(4); bad[0, 3] = np.nan
    with pytest.raises(pkg.LviError) as e:
        g.add_loop(3, 4, bad, 0.1)
    assert e.value.code == -1
    with pytest.raises(pkg.LviError) as e:
        g.add_pose(sc["poses"][-1], sc["poses"][-1])
    assert e.value.code == -4                                          # max_poses
    with pytest.raises(pkg.LviError) as e:
        g.add_pose(None, sc["poses"][-1])
    assert e.value.code == -1
    for frm, to, Zl, var in sc["loops"]:
        g.add_loop(frm, to, Zl, var)
    with pytest.raises(pkg.LviError) as e:
        g.add_loop(10, 20, Z, 0.1)
    assert e.value.code == -4                                          # max_loops
    assert g.count() == twin.count() == (37, 3)
    for bad_kw in (dict(full_logmap=2), dict(max_iters=0), dict(max_iters=pkg.pgo.MAX_ITERS + 1), dict(conv_eps=0.0)):
        with pytest.raises(pkg.LviError) as e:
            g.set_params(**bad_kw)
        assert e.value.code == -1
    with pytest.raises(pkg.LviError):
        g.poses(30, 8)
    ia, ib = g.solve(), twin.solve()
    assert ia == ib
    np.testing.assert_array_equal(g.poses()[0], twin.poses()[0])
    # the soft status: one step cannot converge on this scene
    g.clear()
    assert g.count() == (0, 0)
    R.build(sc, g)
    g.set_params(max_iters=1)
    r = g.solve()
    assert r["status"] == pkg.pgo.NOT_CONVERGED == 1 and not r["converged"] and r["iterations"] == 1 and r["max_step"] > 1e-4
    for bad_create in (dict(max_poses=0), dict(max_poses=pkg.pgo.MAX_POSES + 1), dict(max_loops=-1), dict(max_loops=pkg.pgo.MAX_LOOPS + 1)):
        with pytest.raises(pkg.LviError) as e:
            pkg.PoseGraph(hip, **{**dict(max_poses=8, max_loops=1), **bad_create})
        assert e.value.code == -1
    g.close(); twin.close()


# ---- node level ------------------------------------------------------------------------------------------
SEQ_P = dict(N_SCAN=4, Horizon_SCAN=8192, max_raw_points=20000, max_map_points=600000, max_keyframes=64, max_keyframe_points=600000)


def _rows_to_rpyxyz(rows):
    """lvh_seq_keyposes rows (x y z roll pitch yaw time index) -> (roll, pitch, yaw, x, y, z) float32"""
    return np.ascontiguousarray(rows[:, [3, 4, 5, 0, 1, 2]], F32)


def _map_bits(h):
    from helpers import xyzi
    return [xyzi(c).view(np.uint32).copy() for c in h.get_map_ds()]


def test_pgo_node_applies_the_loop(pkg, hip, oracle):
    """the sequential host node over liblvi_host_hip.so with usePoseGraph on the revisit scene of the loop tests: once the
    loop job's constraint is pushed, the next key solves the graph and correctPoses rewrites every key pose.  The graph's
    poses equal the reference minimiser of the same graph, the node's key poses are their float casts, the device store
    holds them (a fresh store filled with them assembles the same map), lvi_map_update equals lvi_map_assemble bit for
    bit, and a run without usePoseGraph is the odometry chain it was."""
    import loop_scenes as SC
    H = pkg.host_api
    sc = SC.scene("revisit_a", SC.base_passes(pkg, oracle))
    kfs, stamps = sc["kfs"], sc["stamps"]
    n = SC.CUR + 1
    assert len(kfs) == n + 1
    runs = {}
    for with_pg in (False, True):
        m = H.SequentialMapper(pkg.load_host(), hip, pkg.default_params(hip, **SEQ_P), incremental_map=1)
        pg = None
        if with_pg:
            pg = H.PoseGraphBackend(pkg.load_host(), hip, max_poses=64, max_loops=8)
            m.usePoseGraph(pg)
        lc = H.LoopCloser(pkg.load_host(), m, search_radius=15.0, search_time_diff=30.0, search_num=SC.SEARCH, fitness_score=SC.FITNESS_GATE, surf_leaf=SC.LEAF)
        lc.reserve(1 << 16, 1 << 20)
        for k in range(n):
            m.seed_keyframe(kfs[k][0], kfs[k][1], kfs[k][2], stamps[k])
        keys = list(range(n))
        m.handle.map_update(keys)                                         # the local map's sums under the uncorrected poses
        before = m.keyposes()
        pushed, info = lc.performLoopClosure(stamps[n - 1])
        assert pushed and lc.queue_size() == 1
        c = lc.pop()
        if with_pg:
            assert pg.push_loop(c) == 1 and pg.last()["updates"] == 0 and pg.graph.count() == (n, 0)
        assert m.poses_corrected() == 0
        m.seed_keyframe(kfs[n][0], kfs[n][1], kfs[n][2], stamps[n])          # the next key: addOdomFactor, addLoopFactor, update, correctPoses
        after = m.keyposes()
        m.handle.map_update(keys)
        upd = _map_bits(m.handle)
        m.handle.map_assemble(keys)
        asm = _map_bits(m.handle)
        runs[with_pg] = dict(before=before, after=after, upd=upd, asm=asm, c=c, corrected=m.poses_corrected())
        if with_pg:
            runs[True].update(last=pg.last(), graph=pg.graph.poses(), count=pg.graph.count())
        lc.close()
        m.usePoseGraph(None) if with_pg else None
        m.close()
        if pg is not None:
            pg.close()
    a, b = runs[False], runs[True]
    # without the hook: the odometry chain, nothing corrected; with it, nothing differs until the loop is applied
    want = np.array([k[2] for k in kfs], F32)
    np.testing.assert_array_equal(_rows_to_rpyxyz(a["after"]).view(np.uint32), want.view(np.uint32))
    assert a["corrected"] == 0
    np.testing.assert_array_equal(a["before"], b["before"])
    np.testing.assert_array_equal(a["c"]["between"], b["c"]["between"])
    for x, y in zip(a["upd"], a["asm"]):
        np.testing.assert_array_equal(x, y)
    # with it: one update with one loop, converged, every key pose rewritten once
    last = b["last"]
    assert b["corrected"] == 1 and b["count"] == (n + 1, 1)
    assert (last["updates"], last["loops_added"], last["loops_queued"], last["status"]) == (1, 1, 0, 0) and last["converged"]
    np.testing.assert_array_equal(last["pose_to"].view(np.uint32), want[n].view(np.uint32))
    # the reference minimiser of the same graph: the float poses the node handed to addOdomFactor, the constraint it pushed
    ref = R.Graph(1)
    P = _rows_to_rpyxyz(b["before"])
    for k in range(n):
        ref.add_pose(None if k == 0 else P[k - 1], P[k])
    ref.add_pose(P[n - 1], last["pose_to"])
    ref.add_loop(b["c"]["key_cur"], b["c"]["key_pre"], b["c"]["between"], b["c"]["noise"])
    refc = ref.copy()
    ia, ib = ref.solve("lstsq"), refc.solve("chol")
    T, p = b["graph"]
    info = dict(last, status=last["status"])
    _check("node, revisit_a", T, info, ref.poses(), ia, refc.poses(), ib)
    # the node's key poses are the graph's float poses; the newest included
    got = _rows_to_rpyxyz(b["after"])
    np.testing.assert_array_equal(got.view(np.uint32), p.view(np.uint32))
    moved = np.abs(got[:n, 3:] - P[:, 3:]).max()
    print(f"[pgo] node: largest key translation change {moved:.4f} m; loop {b['c']['key_cur']} -> {b['c']['key_pre']}, noise {b['c']['noise']:.4f}")
    assert moved > 1e-4                                                  # far above the float resolution of a pose here (32 m x 2^-23 = 4e-6): the rewrite is visible
    # lvi_map_update after the correction equals lvi_map_assemble, on the node's store and on a fresh store holding the corrected poses
    for x, y in zip(b["upd"], b["asm"]):
        np.testing.assert_array_equal(x, y)
    assert any(not np.array_equal(x, y) for x, y in zip(b["upd"], a["upd"]))
    h = pkg.LidarHotpath(hip, **SEQ_P)
    for k in range(n + 1):
        h.keyframe_add(kfs[k][0], kfs[k][1], got[k])
    h.map_assemble(list(range(n)))
    for x, y in zip(_map_bits(h), b["asm"]):
        np.testing.assert_array_equal(x, y)
    h.close()
