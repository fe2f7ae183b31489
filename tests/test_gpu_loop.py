"""GPU tier: the loop-closure registration (include/lvi_loop.h) against its restatement (loop_ref.py, loop_scenes.py):
the two submaps bit for bit against gmap_ref, one correspondence pass against the exhaustive f32 answer and math.fsum,
the whole job against the float64 reference with the f32 restatement's own distance from it as the yardstick,
run-to-run bits, no interference with the scan path and the global map, the gates and the errors, and the host mirror's
performLoopClosure."""
import math
import threading

import numpy as np
import pytest

import gmap_ref as G
import loop_ref as LR
import loop_scenes as SC
from helpers import bits, small_params, xyzi

pytestmark = pytest.mark.gpu

KF_P = dict(max_keyframes=64, max_keyframe_points=600000)
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def passes(pkg, oracle):
    return SC.base_passes(pkg, oracle)


@pytest.fixture(scope="module")
def ora(pkg, oracle):
    o = pkg.LidarHotpath(oracle, **small_params(max_map_points=1 << 21))
    yield o
    o.close()


def _store(pkg, hip, kfs, **kw):
    h = pkg.LidarHotpath(hip, **small_params(**KF_P, **kw))
    for c, s, p in kfs:
        h.keyframe_add(c, s, p)
    return h


def _loop(pkg, h, ns=1 << 16, nt=1 << 20):
    lp = pkg.LoopIcp(h)
    lp.reserve(ns, nt)
    return lp


def _params(lp, **kw):
    d = dict(search_num=SC.SEARCH, leaf=SC.LEAF, max_corr_dist=SC.MAX_CORR)
    d.update(kw)
    return lp.default_params(**d)


def test_loop_submaps_bit_equal(pkg, hip, ora, passes):
    """source = key cur alone, target = keys pre - n .. pre + n clipped at both ends of the store, each fused corner_k then
    surf_k and filtered once: bit-equal to gmap_ref's fuse + voxel and to lvi_gmap_build of the same keys; at leaf 0.02 the
    overflow rule makes the submap the fused cloud"""
    sc = SC.scene("revisit_a", passes)
    kfs = sc["kfs"]
    h = _store(pkg, hip, kfs)
    lp = _loop(pkg, h)
    g = pkg.GlobalMap(h)
    g.reserve(1 << 20)
    n = len(kfs)
    seen_overflow = set()
    for cur, pre, leaf in ((SC.CUR, SC.PRE, SC.LEAF), (n - 1, 1, SC.LEAF), (n - 1, 0, SC.LEAF), (3, n - 2, SC.LEAF), (SC.CUR, n - 1, 0.1),
                           (SC.CUR, SC.PRE, 0.02)):
        tag = f"cur {cur} pre {pre} leaf {leaf}"
        lp.start(cur, pre, _params(lp, leaf=leaf, max_iters=1))
        r = lp.result()
        refs = SC.submaps_ref(pkg, ora, kfs, cur, pre, leaf)
        for what, ref, nf, nout, ov, keys in ((pkg.loop.SOURCE, refs[0], r["n_source_fused"], r["n_source"], r["overflow_source"], [cur]),
                                              (pkg.loop.TARGET, refs[1], r["n_target_fused"], r["n_target"], r["overflow_target"],
                                               SC.target_keys(pre, n))):
            assert nf == len(ref["fused"]), tag
            assert bool(ov) == ref["overflow"], tag
            exp = xyzi(ref["fused"]) if ref["overflow"] else ref["pts"]
            got = xyzi(lp.fetch(what))
            assert nout == len(exp) == len(got), tag
            np.testing.assert_array_equal(bits(got), bits(exp), err_msg=tag)
            g.build(keys, G.CORNER_SURF, leaf)
            np.testing.assert_array_equal(bits(got), bits(xyzi(g.fetch(pkg.gmap.FILTERED))), err_msg=tag)
            seen_overflow.add(ref["overflow"])
    assert seen_overflow == {False, True}
    h.close()


def _exhaustive_f32(p, t, chunk=128):
    """per query: the lowest index of the smallest f32 distance, that distance, and a function giving d(query i, target j)"""
    idx, d = LR.nn_exhaustive(np.ascontiguousarray(p, F32), np.ascontiguousarray(t, F32), chunk)
    return idx, d


def test_loop_correspondence_pass(pkg, hip, oracle, passes):
    """debug_step under several transforms, one of which pushes part of the source beyond max_corr_dist: every index is the
    exhaustive f32 answer (a differing index only where the two f32 distances are equal), distance bits equal, the kept
    count exact, each double sum within n 2^-53 sum|terms| of math.fsum"""
    sc = SC.scene("revisit_a", passes)
    h = _store(pkg, hip, sc["kfs"])
    lp = _loop(pkg, h)
    max_corr = 3.0
    lp.start(SC.CUR, SC.PRE, _params(lp, max_corr_dist=max_corr, max_iters=1))
    r = lp.result()
    src, tgt = xyzi(lp.fetch(pkg.loop.SOURCE))[:, :3].copy(), xyzi(lp.fetch(pkg.loop.TARGET))[:, :3].copy()
    n = len(src)
    assert n == r["n_source"] >= 300 and len(tgt) == r["n_target"] >= 1000
    max2 = float(F32(max_corr)) ** 2
    transforms = dict(identity=np.eye(4), undo_drift=np.linalg.inv(sc["D"]), small=LR.rpy_matrix(0.7, -0.4, 0.1, 0.01, -0.02, 0.05),
                      pushed_out=LR.rpy_matrix(28.0, 6.0, 0.5, 0.0, 0.0, 0.3), far=LR.rpy_matrix(0.0, 70.0, 0.0, 0.0, 0.0, 0.0))
    cut_seen = False
    for name, T in transforms.items():
        T32 = np.ascontiguousarray(T, F32)
        idx, d, sums = lp.debug_step(T32)
        p = LR.transform(T32, src)
        ri, rd = _exhaustive_f32(p, tgt)
        keep = rd.astype(F64) <= max2
        nk = int(keep.sum())
        print(f"[corr pass] {name}: kept {nk} of {n}, device count {sums[0]}")
        if 0 < nk < n:
            cut_seen = True
        np.testing.assert_array_equal(idx[~keep], -1, err_msg=name)
        assert np.all(np.isinf(d[~keep])), name
        np.testing.assert_array_equal(bits(d[keep]), bits(rd[keep]), err_msg=name)
        differ = np.nonzero(keep & (idx != ri))[0]
        for i in differ:                                               # a cause check: the device's point is exactly as near
            assert 0 <= idx[i] < len(tgt) and LR.sqd(p[i], tgt[idx[i]]) == rd[i], (name, i, idx[i], ri[i])
        assert sums[0] == nk, name
        if nk == 0:
            assert np.all(sums == 0.0)
            continue
        P, Q = p[keep].astype(F64), tgt[idx[keep]].astype(F64)
        terms = [np.ones(nk)] + [P[:, a] for a in range(3)] + [Q[:, a] for a in range(3)] + [P[:, a] * Q[:, b] for a in range(3) for b in range(3)] + [d[keep].astype(F64)]
        for k, t in enumerate(terms):
            exact = math.fsum(t.tolist())
            bound = nk * 2.0 ** -53 * math.fsum(np.abs(t).tolist())
            print(f"[corr pass] {name} sum {k}: |device - fsum| = {abs(sums[k] - exact):.3e}, bound {bound:.3e}")
            assert abs(sums[k] - exact) <= bound, (name, k)
    assert cut_seen, "no transform exercised the max_corr_dist cut"
    h.close()


def _device_job(pkg, lp, **kw):
    lp.start(SC.CUR, SC.PRE, _params(lp, **kw))
    return lp.result()


def test_loop_whole_job_vs_float64(pkg, hip, oracle, ora, passes):
    """every scene: the device at most 4x as far from the float64 reference as the f32 restatement is (the largest such gap
    over the scenes; rotation angle, translation norm, relative fitness), the converged flag equal, the accept / reject
    decision equal, and the reference itself brings the drifted pose closer to the truth"""
    rows = {}
    for name in SC.DRIFTS:
        sc = SC.scene(name, passes)
        refs = SC.submaps_ref(pkg, ora, sc["kfs"], SC.CUR, SC.PRE)
        src, tgt = refs[0]["pts"], refs[1]["pts"]
        assert len(src) >= 300 and len(tgt) >= 1000
        r32, r64 = SC.reference_pair(oracle, src, tgt)
        h = _store(pkg, hip, sc["kfs"])
        lp = _loop(pkg, h)
        r = _device_job(pkg, lp)
        np.testing.assert_array_equal(bits(xyzi(lp.fetch(pkg.loop.SOURCE))), bits(src))
        aligned = xyzi(lp.fetch(pkg.loop.ALIGNED))
        h.close()
        assert r["status"] == pkg.loop.OK and r["n_source"] == len(src) and r["n_target"] == len(tgt)
        yard = SC.gaps(r32["T"], r32["fitness"], r64["T"], r64["fitness"])
        dev = SC.gaps(r["transformation"], r["fitness"], r64["T"], r64["fitness"])
        print(f"[whole job] {name}: f32-vs-f64 gap (rad, m, rel fitness) = {yard}; device-vs-f64 = {dev}; iterations device {r['iterations']} "
              f"f32 {r32['iterations']} f64 {r64['iterations']}; state device {r['convergence_state']} f64 {r64['state']}; "
              f"fitness device {r['fitness']:.9g} f64 {r64['fitness']:.9g}")
        rows[name] = (yard, dev)
        assert r["converged"] == r64["converged"] == r32["converged"], name
        accept64 = r64["converged"] and r64["fitness"] <= SC.FITNESS_GATE
        assert accept64 == SC.ACCEPT[name] and abs(r64["fitness"] - SC.FITNESS_GATE) > 0.1, (name, r64["fitness"])
        assert (r["converged"] and r["fitness"] <= SC.FITNESS_GATE) == accept64, name
        # the aligned cloud is the source under the final transformation
        exp = LR.transform(r["transformation"].astype(F64), src[:, :3].astype(F64))
        assert np.abs(aligned[:, :3] - exp).max() <= 1e-3, name
        if SC.ACCEPT[name]:
            D = sc["D"]
            res = r64["T"] @ D
            assert LR.rot_angle(np.eye(4), res) < 0.25 * LR.rot_angle(np.eye(4), D), name
            assert np.linalg.norm(res[:3, 3]) < 0.25 * np.linalg.norm(D[:3, 3]), name
    bound = [4.0 * max(rows[s][0][k] for s in rows) for k in range(3)]
    print(f"[whole job] bound (4 x the largest f32-vs-f64 gap): {bound}")
    assert all(b > 0 for b in bound), "degenerate yardstick"
    for name, (_, dev) in rows.items():
        for k in range(3):
            assert dev[k] <= bound[k], (name, k, dev[k], bound[k])


def test_loop_cumulative_switch(pkg, hip, oracle, ora, passes):
    """incremental_cloud = 0 (the source under the composed transformation every iteration): the same answer as the float64
    reference run the same way, to the yardstick of the default mode's test"""
    sc = SC.scene("revisit_a", passes)
    refs = SC.submaps_ref(pkg, ora, sc["kfs"], SC.CUR, SC.PRE)
    r32, r64 = SC.reference_pair(oracle, refs[0]["pts"], refs[1]["pts"], incremental_cloud=False)
    h = _store(pkg, hip, sc["kfs"])
    lp = _loop(pkg, h)
    r = _device_job(pkg, lp, incremental_cloud=0)
    h.close()
    yard = SC.gaps(r32["T"], r32["fitness"], r64["T"], r64["fitness"])
    dev = SC.gaps(r["transformation"], r["fitness"], r64["T"], r64["fitness"])
    print(f"[cumulative] f32-vs-f64 {yard}; device-vs-f64 {dev}; iterations {r['iterations']} / {r64['iterations']}")
    assert r["converged"] == r64["converged"]
    for k in range(3):
        assert dev[k] <= 4.0 * yard[k], (k, dev[k], yard[k])


def _all_outputs(pkg, lp):
    r = lp.result()
    out = [np.array([r[k] for k in sorted(r) if k not in ("transformation", "fitness", "mse")], np.int64), bits(r["transformation"]).copy(),
           np.array([r["fitness"], r["mse"]], F64).view(np.uint64)]
    for what in (pkg.loop.SOURCE, pkg.loop.TARGET, pkg.loop.ALIGNED):
        out.append(bits(xyzi(lp.fetch(what))).copy())
    idx, d, sums = lp.debug_step(r["transformation"])
    out += [idx.copy(), bits(d).copy(), sums.view(np.uint64).copy()]
    return out


def test_loop_reproducible(pkg, hip, passes):
    """two jobs on the same input, and a third on a fresh handle: identical bits in every output"""
    sc = SC.scene("revisit_b", passes)
    outs = []
    h = _store(pkg, hip, sc["kfs"])
    lp = _loop(pkg, h)
    for _ in range(2):
        lp.start(SC.CUR, SC.PRE, _params(lp))
        outs.append(_all_outputs(pkg, lp))
    h.close()
    h = _store(pkg, hip, sc["kfs"])
    lp = _loop(pkg, h)
    lp.start(SC.CUR, SC.PRE, _params(lp))
    outs.append(_all_outputs(pkg, lp))
    h.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            np.testing.assert_array_equal(a, b)


def test_loop_fetch_windows(pkg, hip, passes):
    """after one job, a window that starts inside each of the three clouds = that slice of the whole fetch"""
    sc = SC.scene("revisit_a", passes)
    h = _store(pkg, hip, sc["kfs"])
    lp = _loop(pkg, h)
    lp.start(SC.CUR, SC.PRE, _params(lp))
    for what in (pkg.loop.SOURCE, pkg.loop.TARGET, pkg.loop.ALIGNED):
        whole = lp.fetch(what).copy()
        n = len(whole)
        assert n > 16
        first, count = n // 3, n - n // 3 - 5
        got = lp.fetch(what, first, count)
        assert len(got) == count
        np.testing.assert_array_equal(bits(xyzi(got)), bits(xyzi(whole[first:first + count])), err_msg=f"what {what}")
    h.close()


SEQ_P = dict(N_SCAN=4, Horizon_SCAN=8192, max_raw_points=20000, max_map_points=600000, max_keyframes=64, max_keyframe_points=600000)


def _seq_run(pkg, hip, scans, mode):
    """mode: None (scans only), 'inline' (a loop job and a global-map build after every keyframe, results on this thread),
    'thread' (result / fetch of both on a second thread while the next scans run)"""
    H = pkg.host_api
    m = H.SequentialMapper(pkg.load_host(), hip, pkg.default_params(hip, **SEQ_P), incremental_map=1)
    lp = g = None
    if mode:
        lp = pkg.LoopIcp(m.handle); lp.reserve(1 << 16, 1 << 20)
        g = pkg.GlobalMap(m.handle); g.reserve(600000)
    rows, worker, got = [], None, []

    def collect():
        r = lp.result()
        got.append((r["status"], r["n_source"], len(lp.fetch(pkg.loop.ALIGNED)), g.result()["n_out"], len(g.fetch(pkg.gmap.FILTERED))))
    for k, sc in enumerate(scans):
        r = m.scan(sc, 20.0 + 0.2 * k)
        rows.append((bits(r["pose"]).copy(), [xyzi(c).view(np.uint32).copy() for c in m.handle.get_map_ds()] if k > 0 else None))
        if lp and r["saved_keyframe"] and r["n_keyframes"] >= 2:
            if worker is not None:
                worker.join()                                            # start / build may not overlap result / fetch
            nk = r["n_keyframes"]
            lp.start(nk - 1, 0, lp.default_params(search_num=2, leaf=0.4, min_source=0, min_target=0))
            g.build(list(range(nk)), G.CORNER_SURF, 0.05)
            if mode == "inline":
                collect()
            else:
                worker = threading.Thread(target=collect)
                worker.start()
    if worker is not None:
        worker.join()
    m.close()
    return rows, got


def test_loop_no_interference(pkg, hip):
    """twin sequential runs: pose records and the local map bit-identical with and without a loop job and a global-map build
    in flight after every keyframe, and again with result / fetch on a second thread while the main thread runs scans"""
    S = pkg.synth
    n = 14
    poses = [S.loop_pose(0.3 + 0.05 * k, 0.004 * np.sin(k), -0.004 * np.cos(k)) for k in range(n)]
    scans = [S.make_scan(16001, poses[k], 3000 + k) for k in range(n)]
    base, _ = _seq_run(pkg, hip, scans, None)
    ref_got = None
    for mode in ("inline", "thread"):
        rows, got = _seq_run(pkg, hip, scans, mode)
        assert len(got) >= 3, (mode, got)
        assert all(x[0] == pkg.loop.OK and x[1] == x[2] > 0 and x[3] == x[4] > 0 for x in got), got
        if ref_got is None:
            ref_got = got
        assert got == ref_got
        for k in range(n):
            np.testing.assert_array_equal(rows[k][0], base[k][0], err_msg=f"{mode} scan {k}")
            if k > 0:
                for x, y in zip(rows[k][1], base[k][1]):
                    np.testing.assert_array_equal(x, y, err_msg=f"{mode} scan {k}")


def test_loop_gates_and_errors(pkg, hip, passes):
    """the too-few-points statuses, fewer than 3 correspondences, no reservation, capacity, keys out of range and bad
    parameters; an error leaves the previous result readable"""
    L = pkg.loop
    sc = SC.scene("revisit_a", passes)
    kfs = sc["kfs"]
    h = _store(pkg, hip, kfs)
    lp = pkg.LoopIcp(h)
    assert lp.arena_bytes() == 0
    with pytest.raises(pkg.LviError) as e:
        lp.start(SC.CUR, SC.PRE, _params(lp))
    assert e.value.code == -5                                             # LVI_ERR_STATE: no reservation
    with pytest.raises(pkg.LviError) as e:
        lp.result()
    assert e.value.code == -5
    lp.reserve(1 << 16, 1 << 20)
    assert lp.arena_bytes() > 0
    r_ok = _device_job(pkg, lp)
    assert r_ok["status"] == L.OK and r_ok["key_cur"] == SC.CUR and r_ok["key_pre"] == SC.PRE
    # the gates: the source holds fewer points than min_source / the target fewer than min_target
    for kw in (dict(min_source=r_ok["n_source"] + 1), dict(min_target=r_ok["n_target"] + 1)):
        r = _device_job(pkg, lp, **kw)
        assert r["status"] == L.TOO_FEW_POINTS and not r["converged"] and r["iterations"] == 0, kw
        np.testing.assert_array_equal(r["transformation"], np.eye(4, dtype=F32))
        assert len(lp.fetch(L.SOURCE)) == r["n_source"] == r_ok["n_source"]
    r = _device_job(pkg, lp, min_source=r_ok["n_source"], min_target=r_ok["n_target"])
    assert r["status"] == L.OK
    # fewer than 3 correspondences: the source placed 300 m away, nothing within max_corr_dist
    far = [k for k in kfs]
    moved = far[SC.CUR][2].copy(); moved[3] += 300.0
    h2 = _store(pkg, hip, far[:SC.CUR] + [(far[SC.CUR][0], far[SC.CUR][1], moved)] + far[SC.CUR + 1:])
    lp2 = _loop(pkg, h2)
    r = _device_job(pkg, lp2)
    assert r["status"] == L.NO_CORRESPONDENCES and not r["converged"] and r["convergence_state"] == L.CONV_NO_CORRESPONDENCES and r["n_corr"] < 3
    h2.close()
    # errors leave the last result readable
    before = lp.result()
    al_before = bits(xyzi(lp.fetch(L.ALIGNED))).copy()
    n = len(kfs)
    for cur, pre, kw, code in ((n, 0, {}, -1), (-1, 0, {}, -1), (0, n, {}, -1), (0, -1, {}, -1), (SC.CUR, SC.PRE, dict(leaf=-0.1), -1),
                               (SC.CUR, SC.PRE, dict(leaf=float("nan")), -1), (SC.CUR, SC.PRE, dict(max_iters=0), -1),
                               (SC.CUR, SC.PRE, dict(max_corr_dist=0.0), -1), (SC.CUR, SC.PRE, dict(search_num=-1), -1)):
        with pytest.raises(pkg.LviError) as e:
            lp.start(cur, pre, _params(lp, **kw))
        assert e.value.code == code, (cur, pre, kw)
    after = lp.result()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    np.testing.assert_array_equal(bits(xyzi(lp.fetch(L.ALIGNED))), al_before)
    with pytest.raises(pkg.LviError):
        lp.fetch(L.SOURCE, 0, before["n_source"] + 1)
    # capacity: a reservation smaller than a fused submap
    h3 = _store(pkg, hip, kfs)
    lp3 = pkg.LoopIcp(h3)
    lp3.reserve(100, 1 << 20)
    with pytest.raises(pkg.LviError) as e:
        lp3.start(SC.CUR, SC.PRE, _params(lp3))
    assert e.value.code == -4                                             # the source
    lp3.release()                                                         # (a reservation only ever grows)
    lp3.reserve(1 << 16, 1000)
    with pytest.raises(pkg.LviError) as e:
        lp3.start(SC.CUR, SC.PRE, _params(lp3))
    assert e.value.code == -4                                             # the target
    lp3.reserve(1 << 16, 1 << 20)
    assert _device_job(pkg, lp3)["status"] == L.OK
    lp3.release()
    assert lp3.arena_bytes() == 0
    lp3.reserve(1 << 16, 1 << 20)
    lp3.start(SC.CUR, SC.PRE, _params(lp3))
    h3.keyframes_clear()                                                  # waits for the job in flight
    assert lp3.result()["status"] == L.OK
    h3.close()
    h.close()


def test_loop_closer_node(pkg, hip, oracle, ora, passes):
    """the host mirror over liblvi_host_hip.so: a sequence that closes a loop yields one constraint whose indices, between
    pose and noise match the reference pipeline (float64 ICP, float64 constraint) within the bounds of the whole-job
    check; the publishers' clouds are the job's; a second call for the same cur yields none"""
    H, L = pkg.host_api, pkg.loop
    sc = SC.scene("revisit_a", passes)
    kfs, stamps = sc["kfs"], sc["stamps"]
    n = SC.CUR + 1                                                        # the store ends with the key that revisits
    m = H.SequentialMapper(pkg.load_host(), hip, pkg.default_params(hip, **SEQ_P), incremental_map=1)
    lc = H.LoopCloser(pkg.load_host(), m, search_radius=15.0, search_time_diff=30.0, search_num=SC.SEARCH, fitness_score=SC.FITNESS_GATE,
                      surf_leaf=SC.LEAF)
    lc.reserve(1 << 16, 1 << 20)
    assert lc.performLoopClosure(0.0) == (False, None)                    # no key poses yet
    for k in range(n):
        m.seed_keyframe(kfs[k][0], kfs[k][1], kfs[k][2], stamps[k])
    now = stamps[n - 1]
    # the restatement of detectLoopClosureDistance: nearest first, the first more than 30 s away
    P = np.array([k[2][3:6] for k in kfs[:n]], F32)
    d = LR.sqd(P, P[-1])
    order = [i for i in np.argsort(d, kind="stable") if float(d[i]) <= 15.0 ** 2]
    pre = next(i for i in order if abs(stamps[i] - now) > 30.0)
    assert lc.detectLoopClosureDistance(now) == (n - 1, pre)
    cur = n - 1
    refs = SC.submaps_ref(pkg, ora, kfs[:n], cur, pre)
    r32, r64 = SC.reference_pair(oracle, refs[0]["pts"], refs[1]["pts"])
    assert r64["converged"] and r64["fitness"] <= SC.FITNESS_GATE
    pose6 = lambda p: np.asarray(p, F64)                                  # (roll, pitch, yaw, x, y, z)
    ref_between = LR.constraint(r64["T"], pose6(kfs[cur][2]), pose6(kfs[pre][2]))
    f32_between = LR.constraint(r32["T"].astype(F64), pose6(kfs[cur][2]), pose6(kfs[pre][2]))
    pushed, info = lc.performLoopClosure(now)
    assert pushed and info["status"] == L.OK and info["converged"]
    assert lc.queue_size() == 1 and lc.closed() == {cur: pre}
    c = lc.pop()
    assert (c["key_cur"], c["key_pre"]) == (cur, pre) and lc.queue_size() == 0 and lc.pop() is None
    yard = SC.gaps(f32_between, r32["fitness"], ref_between, r64["fitness"])
    dev = SC.gaps(c["between"], c["noise"], ref_between, r64["fitness"])
    print(f"[loop closer] between: f32 pipeline vs float64 {yard}; mirror vs float64 {dev}")
    assert c["noise"] == float(F32(info["fitness"]))
    # the bounds of the whole-job check, plus what the constraint's own f32 steps (tWrong, tCorrect, its Euler angles) add:
    # 2^-23 relative on a pose of |t| <= 32 m and angles <= pi, a few operations
    extra_t, extra_r = 32.0 * 2.0 ** -23 * 8, np.pi * 2.0 ** -23 * 8
    assert dev[0] <= 4.0 * yard[0] + extra_r and dev[1] <= 4.0 * yard[1] + extra_t and dev[2] <= 4.0 * yard[2] + 2.0 ** -23, (dev, yard)
    # the publishers' clouds
    np.testing.assert_array_equal(bits(xyzi(lc.cloud(L.TARGET))), bits(refs[1]["pts"]))
    al = xyzi(lc.cloud(L.ALIGNED))
    assert np.abs(al[:, :3] - LR.transform(info["transformation"].astype(F64), refs[0]["pts"][:, :3].astype(F64))).max() <= 1e-3
    # the same cur again: already closed
    assert lc.detectLoopClosureDistance(now) is None
    assert lc.performLoopClosure(now) == (False, None) and lc.queue_size() == 0
    lc.close()
    m.close()
