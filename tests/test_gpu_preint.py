"""GPU tier of the IMU preintegration (include/lvi_preint.h) against tests/preint_ref.py.

The device runs only IEEE + - * / sqrt in the order csrc/lvi_preint_math.hpp states, with contraction off, so every
comparison with the float64 reference is equality of bits (np.array_equal: -0.0 == 0.0) on every field of the record and on
the navigation state; there is no tolerance to choose.  lvi_preint_evaluate is csrc/lvi_imu_math.hpp on the host and is held
to the bar tests/test_win_ref.py holds that header to.  The handle holds 2 LVI_PREINT_CHUNK + 3 samples per slot, so every
chunk edge is met with a few dozen samples."""
import os
import subprocess

import numpy as np
import pytest

import fman_ref as FR
import marg_ref as M
import preint_ref as R
import win_ref as W
import win_scenes as S

pytestmark = pytest.mark.gpu

CHUNK = R.CHUNK
CAP = 2 * CHUNK + 3
U = 2.0 ** -53
FIELDS = ("sum_dt", "delta_p", "delta_q", "delta_v", "linearized_ba", "linearized_bg", "jacobian", "covariance")
NAV0 = dict(P=np.array([0.3, -0.1, 0.2]), R=M.rot(M.rand_quat(np.random.RandomState(5), 0.3)), V=np.array([1.5, 0.2, -0.1]),
            Ba=np.array([0.01, -0.02, 0.015]), Bg=np.array([0.001, 0.002, -0.0015]))


@pytest.fixture(scope="module")
def win(pkg, hip):
    w = pkg.ImuWindow(hip, max_samples=CAP)
    yield w
    w.close()


def _rec(r):
    """a one-element IMU_DTYPE array -> the reference's dict"""
    assert all(int(r[k][0]) == 0 for k in ("pose_i", "speed_bias_i", "pose_j", "speed_bias_j"))
    return {k: (float(r[k][0]) if k == "sum_dt" else np.array(r[k][0])) for k in FIELDS}


def _exists(pkg, w, slot):
    try:
        w.count(slot)
        return True
    except pkg.LviError as e:
        assert e.code == pkg._abi.LVI_ERR_STATE
        return False


def _same(pkg, w, est, what, slots=range(R.SLOTS)):
    """every slot's existence, record and samples, and the navigation state, against the reference"""
    for i in slots:
        assert _exists(pkg, w, i) == (est.slots[i] is not None), (what, i)
        if est.slots[i] is None:
            continue
        diff = R.same_record(_rec(w.record(i)), est.record(i))
        assert diff is None, f"{what}: slot {i}: {diff}"
        assert all(np.array_equal(a, b) for a, b in zip(w.samples(i), est.samples(i))), (what, i, "samples")
    got, want = w.nav(), est.nav_f64()
    for k in ("P", "R", "V", "Ba", "Bg"):
        assert np.array_equal(got[k], want[k]), (what, "nav", k, got[k], want[k])


def _state(pkg, w):
    """the full download as bytes"""
    out = []
    for i in range(R.SLOTS):
        if _exists(pkg, w, i):
            out += [w.record(i).tobytes()] + [a.tobytes() for a in w.samples(i)]
        else:
            out.append(None)
    n = w.nav()
    return out + [n[k].tobytes() for k in ("P", "R", "V", "Ba", "Bg")]


def _start(w, nav=NAV0, **params):
    w.clear()
    w.set_nav(**nav)
    est = R.Estimator(max_samples=CAP, **params)
    est.set_nav(**nav)
    return est


def _both(w, est, frame_count, dt, acc, gyr):
    w.push(frame_count, dt, acc, gyr)
    est.push(frame_count, dt, acc, gyr)


# ---- sample counts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, CHUNK - 1, CHUNK, CHUNK + 1, CAP])
def test_sample_counts(pkg, win, n):
    dt, acc, gyr = R.samples(40 + n, n + 1, vary=True)
    est = _start(win)
    _both(win, est, 0, dt[:1], acc[:1], gyr[:1])
    _both(win, est, 10, dt[1:], acc[1:], gyr[1:])
    assert _exists(pkg, win, 10) == (n > 0) and _exists(pkg, win, 0) and not _exists(pkg, win, 5)
    if n:
        assert win.count(10) == n
        print(f"[preint gpu] {n} samples: sum_dt {float(win.record(10)['sum_dt'][0])!r}, nav P {win.nav()['P']}")
    _same(pkg, win, est, f"{n} samples")


def test_the_split_into_pushes_and_the_slot_do_not_matter(pkg, win):
    dt, acc, gyr = R.samples(77, CAP + 1, vary=True, zero_dt_at=9)
    results = {}
    for name, slot, cuts in (("one at a time", 10, list(range(1, CAP + 2))), ("1, CHUNK, rest", 10, [1, 2, 2 + CHUNK, CAP + 1]), ("at once", 10, [1, CAP + 1]),
                             ("at once in slot 1", 1, [1, CAP + 1])):
        est = _start(win)
        win.push(0, dt[:1], acc[:1], gyr[:1])
        for a, b in zip(cuts[:-1], cuts[1:]):
            win.push(slot, dt[a:b], acc[a:b], gyr[a:b])
        n = win.nav()
        results[name] = [win.record(slot).tobytes()] + [x.tobytes() for x in win.samples(slot)] + [n[k].tobytes() for k in ("P", "R", "V")]
        assert win.count(slot) == CAP
    est.push(0, dt[:1], acc[:1], gyr[:1])
    est.push(1, dt[1:], acc[1:], gyr[1:])
    _same(pkg, win, est, "at once in slot 1")
    for name in results:
        assert results[name] == results["at once"], name


def test_slot_0_and_first_use(pkg, win):
    dt, acc, gyr = R.samples(78, 7)
    est = _start(win)
    _both(win, est, 0, dt[:3], acc[:3], gyr[:3])           # frame_count == 0: slot 0 is created from the FIRST sample and integrates nothing
    assert win.count(0) == 0 and float(win.record(0)["sum_dt"][0]) == 0.0
    assert np.array_equal(win.record(0)["jacobian"][0], np.eye(15)) and not win.record(0)["covariance"].any()
    assert np.array_equal(win.nav()["P"], NAV0["P"])       # the navigation state did not move
    _same(pkg, win, est, "frame_count 0")
    _both(win, est, 1, dt[3:], acc[3:], gyr[3:])           # slot 1 starts from acc_0 = the third sample
    assert win.count(1) == 4
    _same(pkg, win, est, "frame_count 1")
    # the same samples without the first three: another acc_0, another record
    est2 = _start(win)
    _both(win, est2, 1, dt[3:], acc[3:], gyr[3:])
    _same(pkg, win, est2, "first sample ever in slot 1")
    assert R.same_record(est2.record(1), est.record(1)) is not None


# ---- repropagate -------------------------------------------------------------------------------------------------
COUNTS = [3, 1, CHUNK, CHUNK + 1, 5, 2, CAP, 7, CHUNK - 1, 4]          # samples of slots 1..10


def _fill(w, seed=90):
    est = _start(w)
    dt, acc, gyr = R.samples(seed, 2)
    _both(w, est, 0, dt, acc, gyr)
    for j, n in enumerate(COUNTS, start=1):
        dt, acc, gyr = R.samples(seed + j, n, vary=True)
        _both(w, est, j, dt, acc, gyr)
        nav = {k: v + 1e-3 * j for k, v in NAV0.items() if k != "R"}            # every slot is created with other biases
        w.set_nav(R=NAV0["R"], **nav)
        est.set_nav(R=NAV0["R"], **nav)
    return est


@pytest.mark.parametrize("slots", [[6], [1, 4, 9], list(range(R.SLOTS))])
def test_repropagate(pkg, win, slots):
    est = _fill(win)
    _same(pkg, win, est, "filled")
    before = _state(pkg, win)
    rs = np.random.RandomState(len(slots))
    Bas, Bgs = rs.normal(0, 0.02, (R.SLOTS, 3)), rs.normal(0, 0.002, (R.SLOTS, 3))
    win.repropagate(Bas, Bgs, slots)
    est.repropagate(Bas, Bgs, slots)
    _same(pkg, win, est, f"repropagate {slots}")
    after = _state(pkg, win)
    pos, k = {}, 0
    for i in range(R.SLOTS):
        pos[i] = k
        k += 4
    for i in range(R.SLOTS):
        same = after[pos[i]:pos[i] + 4] == before[pos[i]:pos[i] + 4]
        assert same == (i not in slots), (i, same)       # a slot in the mask changed (its biases did), the others kept their bytes
    assert after[k:] == before[k:]                                             # the navigation state too
    if len(slots) == R.SLOTS:
        # one launch of eleven jobs equals eleven launches of one
        _fill(win)
        for i in slots:
            win.repropagate(Bas, Bgs, [i])
        assert _state(pkg, win) == after
        # and with a slot's own biases the record comes back bit for bit
        own_a = np.array([_rec(win.record(i))["linearized_ba"] for i in range(R.SLOTS)])
        own_g = np.array([_rec(win.record(i))["linearized_bg"] for i in range(R.SLOTS)])
        win.repropagate(own_a, own_g)
        assert _state(pkg, win) == after


# ---- the slides --------------------------------------------------------------------------------------------------
def test_slides_over_14_images(pkg, win):
    """images 0..10 fill the window; then new (the merge crosses a chunk boundary: 10 + 10), new (it fills slot 9 exactly:
    20 + 15 = 2 CHUNK + 3), old, new"""
    per_image = [2, 3, 4, 5, 6, 3, 2, 4, 5, 10, 10, 15, 6, 4]
    flags = {10: "new", 11: "new", 12: "old", 13: "new"}
    est, frame_count = _start(win), 0
    rs = np.random.RandomState(3)
    for image, n in enumerate(per_image):
        dt, acc, gyr = R.samples(200 + image, n, vary=True)
        for k in range(n):
            win.process_imu(dt[k], acc[k], gyr[k])
        win.flush(frame_count)
        est.push(frame_count, dt, acc, gyr)
        _same(pkg, win, est, f"image {image}, push")
        if frame_count < R.WINDOW:
            frame_count += 1
            continue
        nav = dict(P=rs.normal(0, 1, 3), R=M.rot(M.rand_quat(rs, 0.5)), V=rs.normal(0, 1, 3), Ba=rs.normal(0, 0.02, 3), Bg=rs.normal(0, 0.002, 3))
        win.set_nav(**nav)                                  # double2vector, before the slide
        est.set_nav(**nav)
        c9, c10 = win.count(9), win.count(10)
        if flags[image] == "old":
            win.slide_old()
            est.slide_old()
        else:
            win.slide_new()
            est.slide_new()
            assert win.count(9) == c9 + c10
            if image == 10:
                assert c9 < CHUNK < c9 + c10
            if image == 11:
                assert c9 + c10 == CAP
        assert win.count(10) == 0 and np.array_equal(win.record(10)["linearized_ba"][0], nav["Ba"])
        print(f"[preint gpu] image {image}: slide {flags[image]}, slot 9 {c9} -> {win.count(9)} samples, slot 10 {c10} -> 0")
        _same(pkg, win, est, f"image {image}, slide {flags[image]}")


# ---- errors leave the state unchanged -----------------------------------------------------------------------------------
def test_errors_leave_the_state_unchanged(pkg, hip, win):
    E = pkg._abi
    est = _fill(win)
    before = _state(pkg, win)
    dt, acc, gyr = R.samples(7, 3)
    bad = lambda a, k: np.where(np.arange(a.size).reshape(a.shape) == k, np.nan, a)
    cases = [("frame_count -1", lambda: win.push(-1, dt, acc, gyr), E.LVI_ERR_INVALID_ARG),
             ("frame_count 11", lambda: win.push(11, dt, acc, gyr), E.LVI_ERR_INVALID_ARG),
             ("n < 0", lambda: win._call("lvi_preint_push", 3, -1, None, None, None), E.LVI_ERR_INVALID_ARG),
             ("dt nan", lambda: win.push(3, bad(dt, 1), acc, gyr), E.LVI_ERR_INVALID_ARG),
             ("acc inf", lambda: win.push(3, dt, np.where(np.isnan(bad(acc, 4)), np.inf, acc), gyr), E.LVI_ERR_INVALID_ARG),
             ("gyr nan", lambda: win.push(3, dt, acc, bad(gyr, 8)), E.LVI_ERR_INVALID_ARG),
             ("push over capacity", lambda: win.push(7, dt[:1], acc[:1], gyr[:1]), E.LVI_ERR_CAPACITY),        # slot 7 is full
             ("get of slot 11", lambda: win.record(11), E.LVI_ERR_INVALID_ARG),
             ("repropagate with a nan bias", lambda: win.repropagate(bad(np.zeros((11, 3)), 2), np.zeros((11, 3))), E.LVI_ERR_INVALID_ARG)]
    assert win.count(7) == CAP
    for name, call, code in cases:
        with pytest.raises(pkg.LviError) as e:
            call()
        assert e.value.code == code, name
        assert _state(pkg, win) == before, name
    # slide_new that exceeds capacity: slot 9 holds CHUNK - 1, slot 10 holds 4; fill slot 10 first
    n = CAP - (CHUNK - 1) + 1 - 4
    d2, a2, g2 = R.samples(8, n)
    _both(win, est, 10, d2, a2, g2)
    before = _state(pkg, win)
    with pytest.raises(pkg.LviError) as e:
        win.slide_new()
    assert e.value.code == E.LVI_ERR_CAPACITY and _state(pkg, win) == before
    with pytest.raises(R.CapacityError):
        est.slide_new()
    _same(pkg, win, est, "after the refused calls")
    # slots that do not exist
    win.clear()
    win.set_nav(**NAV0)
    win.push(2, dt, acc, gyr)
    before = _state(pkg, win)
    for name, call in (("repropagate", lambda: win.repropagate(np.zeros((11, 3)), np.zeros((11, 3)), [2, 3])), ("get", lambda: win.record(3)),
                       ("samples", lambda: win.samples(3)), ("slide_new", lambda: win.slide_new()),
                       ("evaluate", lambda: win.evaluate(3, np.r_[0, 0, 0, 0, 0, 0, 1.0], np.zeros(9), np.r_[0, 0, 0, 0, 0, 0, 1.0], np.zeros(9)))):
        with pytest.raises(pkg.LviError) as e:
            call()
        assert e.value.code == E.LVI_ERR_STATE, name
        assert _state(pkg, win) == before, name
    # bad caps at create
    for cap in (0, -3, pkg.preint.MAX_SAMPLES + 1):
        with pytest.raises(pkg.LviError) as e:
            pkg.ImuWindow(hip, max_samples=cap)
        assert e.value.code == E.LVI_ERR_INVALID_ARG and "max_samples is outside 1..LVI_PREINT_MAX_SAMPLES" in str(e.value)


# ---- lvi_preint_evaluate ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [31, 32])
def test_evaluate_against_the_imu_factor_reference(pkg, win, seed):
    """bar (as tests/test_win_ref.py holds csrc/lvi_imu_math.hpp to): max(10 G, 15 u x the largest entry), G the float64-to-mpmath
    distance of win_ref.imu_factor for that case"""
    rs = np.random.RandomState(seed)
    ba, bg, intervals = R.scene_intervals(seed, 2)
    dts, accs, gyrs, _ = intervals[0]
    win.clear()
    win.set_nav(P=np.zeros(3), R=np.eye(3), V=np.zeros(3), Ba=ba, Bg=bg)
    win.push(0, dts[:1], accs[:1], gyrs[:1])
    win.push(1, dts[1:], accs[1:], gyrs[1:])
    rec = _rec(win.record(1))
    dt = rec["sum_dt"]
    G = np.array([0.0, 0.0, 9.8])
    pose_i = np.r_[rs.normal(0, 0.5, 3), M.rand_quat(rs, 0.3)]
    sb_i = np.r_[rs.normal(0, 1, 3), ba + rs.normal(0, 1e-3, 3), bg + rs.normal(0, 1e-4, 3)]
    Ri = M.rot(pose_i[3:])
    pose_j = np.r_[pose_i[:3] + sb_i[:3] * dt - 0.5 * G * dt * dt + Ri @ rec["delta_p"] + rs.normal(0, 1e-2, 3),
                   M.quat_mul(M.quat_mul(pose_i[3:], rec["delta_q"]), M.rand_quat(rs, 1e-2))]
    sb_j = np.r_[sb_i[:3] - G * dt + Ri @ rec["delta_v"] + rs.normal(0, 1e-2, 3), sb_i[3:6] + rs.normal(0, 1e-4, 3), sb_i[6:9] + rs.normal(0, 1e-5, 3)]
    r, J = win.evaluate(1, pose_i, sb_i, pose_j, sb_j)
    assert not J[0][:, 6].any() and not J[2][:, 6].any()
    got = np.concatenate([r, np.hstack([J[0][:, :6], J[1], J[2][:, :6], J[3]]).ravel()])
    ref = []
    for X in (W.F64, W.MP):
        rr, JJ = W.imu_factor(pose_i, sb_i, pose_j, sb_j, rec, G, X)
        ref.append(np.concatenate([rr, JJ.ravel()]))
    Gd = M.gap(ref[0], ref[1])
    tol = max(10 * Gd, 15 * U * float(np.abs(ref[0]).max()))
    err = float(np.abs(got - ref[0]).max())
    print(f"[preint gpu] evaluate seed {seed}: G {Gd:.3e}, bar {tol:.3e}, error {err:.3e}, largest entry {np.abs(ref[0]).max():.3e}")
    assert err <= tol


# ---- lifecycle ----------------------------------------------------------------------------------------------------------
def test_create_and_destroy_repeatedly(pkg, hip):
    import torch
    pkg.ImuWindow(hip, max_samples=CAP).close()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(30):
        w = pkg.ImuWindow(hip, max_samples=CAP)
        w.close()
        w.close()
    pkg.ImuWindow(hip, max_samples=1).close()
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    arena = R.SLOTS * (56 * CAP + 3832)
    print(f"[preint gpu] free before {before}, after {after}, arena >= {arena}")
    assert after >= before - arena


def test_two_handles_interleaved_equal_one_alone(pkg, hip):
    def steps():
        dt, acc, gyr = R.samples(300, 2)
        yield lambda w: (w.clear(), w.set_nav(**NAV0), w.push(0, dt, acc, gyr))
        for j in range(1, R.SLOTS):
            d, a, g = R.samples(300 + j, 3 + j, vary=True)
            yield lambda w, j=j, d=d, a=a, g=g: w.push(j, d, a, g)
        yield lambda w: w.slide_new()
        yield lambda w: w.repropagate(np.full((11, 3), 0.01), np.full((11, 3), 0.001), [2, 9])
        yield lambda w: w.slide_old()
    a, b = pkg.ImuWindow(hip, max_samples=CAP), pkg.ImuWindow(hip, max_samples=CAP)
    try:
        for st in steps():
            st(a)
            st(b)
        ra, rb = _state(pkg, a), _state(pkg, b)
    finally:
        b.close()
        a.close()
    c = pkg.ImuWindow(hip, max_samples=CAP)
    try:
        for st in steps():
            st(c)
        rc = _state(pkg, c)
    finally:
        c.close()
    assert ra == rb == rc and sum(x is not None for x in rc) > 20


# ---- the chain with IMU -------------------------------------------------------------------------------------------------------
CHAIN_SEED, CHAIN_STILL = 6, (10, 12)
G3 = np.array([0.0, 0.0, 9.8])


def _rotvec(Rm):
    q = FR.rot_to_quat(Rm)
    s = np.linalg.norm(q[:3])
    return np.zeros(3) if s < 1e-300 else 2.0 * np.arctan2(s, q[3]) * q[:3] / s


def _chain_imu(seq, rs):
    """IMU samples that carry the sequence's poses: S.FRAME_SAMPLES samples of S.SAMPLE_DT per interval, a constant world
    acceleration and body rate per interval, drawn with the noise tests/win_scenes.py::make_scene draws
    -> (velocities [n, 3], per interval (dt, acc, gyr))"""
    Ps, Rs = seq["Ps"], seq["Rs"]
    T = S.FRAME_SAMPLES * S.SAMPLE_DT
    v = [(Ps[1] - Ps[0]) / T]
    for i in range(len(Ps) - 1):
        v.append(2 * (Ps[i + 1] - Ps[i]) / T - v[i])
    out = []
    for i in range(len(Ps) - 1):
        a0, w0 = Rs[i].T @ ((v[i + 1] - v[i]) / T + G3), _rotvec(Rs[i].T @ Rs[i + 1]) / T
        out.append((np.full(S.FRAME_SAMPLES, S.SAMPLE_DT), np.array([a0 + rs.normal(0, 0.05, 3) for _ in range(S.FRAME_SAMPLES)]),
                    np.array([w0 + rs.normal(0, 0.01, 3) for _ in range(S.FRAME_SAMPLES)])))
    return np.array(v), out


def _as_array(pkg, rec):
    r = np.zeros(1, pkg.win.IMU_DTYPE)
    for k in FIELDS:
        r[k][0] = rec[k]
    return r


def test_chain_of_14_frames_with_imu(pkg, hip):
    """tests/test_gpu_fman.py::test_chain_of_14_frames with the IMU in it: processIMU per interval, the ten records into the
    window solve, pre_integrations[1] into the marginaliser, both slides.  On every solved image the device's records equal the
    reference's, the solve fed with either returns the same bytes, it meets no bad covariance, lowers the cost and holds ten
    IMU factors, and MARGIN_OLD keeps a speed-bias block, which only the IMU factor names."""
    H = pkg.host_api
    hl = pkg.load_host()
    seq = FR.sequence(CHAIN_SEED, n_frames=14, per_frame=60, still=CHAIN_STILL, step=0.3)
    rs = np.random.RandomState(1)
    tic, ric, td = seq["tic"], seq["ric"], 0.002
    ex = np.r_[tic, FR.rot_to_quat(ric)]
    vel, imu = _chain_imu(seq, rs)

    def guess(i):                                          # the state a front end would hand in: the truth, slightly off
        return (np.r_[seq["Ps"][i] + rs.normal(0, 0.005, 3), FR.rot_to_quat(seq["Rs"][i] @ FR.rot(rs.normal(0, 1, 3), 0.002))],
                np.r_[vel[i] + rs.normal(0, 0.01, 3), rs.normal(0, 1e-3, 3), rs.normal(0, 1e-4, 3)])

    pkg.win.bind(hip)
    FM = H.FeatureManager(hl, hip, max_features=512)
    V = H.VinsMarginalizer(hl, hip, max_features=200, estimate_td=True)
    O = H.VinsWindowOptimizer(hl, hip, V, max_features=200, estimate_extrinsic=0, num_iterations=8, solver_time=0.0)
    IW = pkg.ImuWindow(hip, max_samples=CAP)
    est = R.Estimator(max_samples=CAP)
    fm, poses, sbs, slides, frame_count, prior_n = FR.FeatureManager(), [], [], [], 0, 0
    try:
        for i, (ids, obs) in enumerate(seq["frames"]):
            p, sb = guess(i)
            poses.append(p)
            sbs.append(sb)
            if i == 0:
                nav0 = dict(P=p[:3], R=FR.quat_to_rot(p[3:]), V=sb[:3], Ba=sb[3:6], Bg=sb[6:9])
                IW.set_nav(**nav0)
                est.set_nav(**nav0)
                d, a, g = (x[:1] for x in imu[0])            # the sample that arrives with the first image
            else:
                d, a, g = imu[i - 1]
            for k in range(len(d)):
                IW.process_imu(d[k], a[k], g[k])
            IW.flush(frame_count)
            est.push(frame_count, d, a, g)
            info = FM.add_frame(frame_count, ids, obs, td)
            fm.add_frame(frame_count, ids, obs, td)
            if frame_count < R.WINDOW:
                frame_count += 1
                continue
            Ps = np.array([q[:3] for q in poses])
            Rs = np.array([FR.quat_to_rot(q[3:]) for q in poses])
            FM.triangulate(Ps, Rs, tic, ric)
            got = {int(f["feature_id"]): float(f["estimated_depth"]) for f in FM.table.download()}
            fm.triangulate(Ps, Rs, tic, ric, depth_of=lambda f: got[f.feature_id])
            flag = V.MARGIN_OLD if info["keyframe"] else V.MARGIN_SECOND_NEW
            # (i) the device's ten records equal the reference's
            dev = {j: IW.record(j) for j in range(1, R.SLOTS)}
            for j in range(1, R.SLOTS):
                diff = R.same_record(_rec(dev[j]), est.record(j))
                assert diff is None, f"image {i}, slot {j}: {diff}"
                assert IW.count(j) == len(est.slots[j]["samples"]) > 0

            def solve(records):
                V.set_window(np.array(poses), np.array(sbs), ex, td)
                FM.fill_window(V, O)
                for j in range(1, R.SLOTS):
                    O.set_imu(j, records[j])
                sol = O.optimize(flag)
                return sol, O.window()
            # (ii) the same library fed the same bytes: the reference's records, then the device's through ImuWindow.fill
            sol_r, out_r = solve({j: _as_array(pkg, est.record(j)) for j in range(1, R.SLOTS)})
            V.set_window(np.array(poses), np.array(sbs), ex, td)
            FM.fill_window(V, O)
            IW.fill(O)
            sol, out = O.optimize(flag), O.window()
            for k in ("pose", "speed_bias", "ex_pose", "inv_dep"):
                assert out[k].tobytes() == out_r[k].tobytes(), (i, k)
            assert out["td"] == out_r["td"] and all(sol[k] == sol_r[k] for k in sol if k != "time_s"), (sol, sol_r)
            # (iii) no bad covariance, a lower cost, ten IMU factors
            D, E, rows = (pkg.win.C.c_int32(0) for _ in range(3))
            hip.check(hip.dll.lvi_win_debug_system(pkg.win.C.c_void_p(hl.dll.lvh_win_handle(O._p)), 0, 0, 0, 0, pkg.win.C.byref(D), pkg.win.C.byref(E),
                                                   pkg.win.C.byref(rows), None, None, None, None, None, None, None, None), "lvi_win_debug_system")
            n_imu = (rows.value - prior_n) / 15
            print(f"[preint gpu] chain image {i}: flag {flag}, solve status {sol['status']}, flags {sol['flags']}, cost {sol['initial_cost']:.4g} -> "
                  f"{sol['final_cost']:.4g} in {sol['iterations']} iterations, {rows.value} dense rows, prior {prior_n}: {n_imu} IMU factors")
            assert sol["status"] == 0 and sol["flags"] == 0 and sol["final_cost"] < sol["initial_cost"] and n_imu == 10
            FM.take_depths(V)
            fm.set_depth([out["inv_dep"][k] for k, f in enumerate(fm.feature) if FR.eligible(len(f.obs), f.start_frame)])
            poses = [out["pose"][k].copy() for k in range(R.SLOTS)]
            sbs = [out["speed_bias"][k].copy() for k in range(R.SLOTS)]
            # (iv) the marginalisation with pre_integrations[1]
            IW.fill_marginalizer(V, out["pose"], out["speed_bias"])
            ran = V.run(flag)
            if ran["ran"]:
                prior_n = ran["n"]
            print(f"[preint gpu] chain image {i}: marginalisation ran {ran['ran']}, status {ran['status']}, m {ran['m']}, n {ran['n']}")
            nav = dict(P=poses[10][:3], R=FR.quat_to_rot(poses[10][3:]), V=sbs[10][:3], Ba=sbs[10][3:6], Bg=sbs[10][6:9])
            IW.set_nav(**nav)                               # double2vector, before the slide
            est.set_nav(**nav)
            if flag == V.MARGIN_OLD:
                assert ran["ran"] and 9 in V.marg.layout()["sizes"].tolist()
                back_R0, back_P0, Rs0, Ps0 = FR.quat_to_rot(poses[0][3:]), poses[0][:3], FR.quat_to_rot(poses[1][3:]), poses[1][:3]
                FM.slide_old(True, back_R0, back_P0, Rs0, Ps0, ric, tic)
                fm.remove_back_shift_depth(*FR.slide_old_frames(back_R0, back_P0, Rs0, Ps0, ric, tic))
                IW.slide_old()
                est.slide_old()
                del poses[0], sbs[0]
            else:
                FM.slide_new(frame_count)
                fm.remove_front(frame_count)
                IW.slide_new()
                est.slide_new()
                del poses[R.WINDOW - 1], sbs[R.WINDOW - 1]
            slides.append(flag)
            _same(pkg, IW, est, f"chain image {i}, slide")
            FM.remove_failures()
            fm.remove_failures()
        print(f"[preint gpu] chain: slides {slides}")
        assert len(slides) == 4 and V.MARGIN_OLD in slides and V.MARGIN_SECOND_NEW in slides
    finally:
        IW.close()
        O.close()
        V.close()
        FM.close()


# ---- lidar_initialise -------------------------------------------------------------------------------------------------------
def test_lidar_initialise(pkg, hip, win):
    sc = FR.window_scene(12, 60)
    frames_obs = [(ids, np.asarray(obs, np.float64).reshape(-1, 8)) for ids, obs in sc["frames"]]
    rs = np.random.RandomState(8)
    frames = [dict(reset_id=3, T=sc["Ps"][i], R=sc["Rs"][i], V=rs.normal(0, 1, 3), Ba=rs.normal(0, 0.02, 3), Bg=rs.normal(0, 0.002, 3), gravity=9.81)
              for i in range(R.SLOTS)]
    tab, twin = pkg.FeatureTable(hip, max_features=128), pkg.FeatureTable(hip, max_features=128)
    try:
        for t in (tab, twin):
            for i, (ids, obs) in enumerate(frames_obs):
                t.add_frame(i, ids, obs, 0.0)
            t.triangulate(sc["Ps"], sc["Rs"], sc["tic"], sc["ric"])
        est = _fill(win)
        # a frame without lidar odometry, and one from another reset: None, and nothing changes
        before, table = _state(pkg, win), tab.download().tobytes()
        for k, rid in ((4, -1), (7, 5)):
            bad = [dict(f) for f in frames]
            bad[k]["reset_id"] = rid
            assert win.lidar_initialise(tab, bad, ric=sc["ric"]) is None
            assert _state(pkg, win) == before and tab.download().tobytes() == table
        out = win.lidar_initialise(tab, frames, ric=sc["ric"])
        Ps, Rs, Vs, Bas, Bgs, g = out
        for got, key in ((Ps, "T"), (Rs, "R"), (Vs, "V"), (Bas, "Ba"), (Bgs, "Bg")):
            assert np.array_equal(got, np.array([f[key] for f in frames]))
        assert np.array_equal(g, [0.0, 0.0, 9.81])
        est.repropagate(Bas, Bgs)                           # every slot repropagated with the frames' biases
        _same(pkg, win, est, "lidar_initialise")
        # :253: the handle's G is g from now on: the next navigation step and lvi_preint_evaluate read it
        assert tuple(win.params.G) == (0.0, 0.0, 9.81)
        est.P["G"] = (0.0, 0.0, 9.81)
        d3, a3, g3 = R.samples(91, 3, vary=True)
        _both(win, est, 10, d3, a3, g3)
        _same(pkg, win, est, "a push after lidar_initialise")
        blocks = (np.r_[0.1, 0.2, 0.3, 0, 0, 0, 1.0], np.r_[1.0, 0, 0, Bas[0], Bgs[0]], np.r_[0.2, 0.2, 0.3, 0, 0, 0, 1.0], np.r_[1.0, 0, 0, Bas[1], Bgs[1]])
        r_new = win.evaluate(1, *blocks)[0]
        win.set_params(G=(0.0, 0.0, 9.8))
        r_old = win.evaluate(1, *blocks)[0]
        assert not np.array_equal(r_new, r_old)
        assert all(np.array_equal(_rec(win.record(i))["linearized_bg"], Bgs[i]) for i in range(R.SLOTS))
        # the table: every depth cleared, then triangulated with tic = 0: the same calls made by hand give the same bytes
        n = len(twin.depth_vector())
        twin.clear_depth(np.full(n, -1.0))
        cleared = twin.download()
        assert n > 20 and all(f["estimated_depth"] == -1.0 and f["lidar_depth_flag"] == 0 for f in cleared if FR.eligible(int(f["n_obs"]), int(f["start_frame"])))
        info = twin.triangulate(Ps, Rs, np.zeros(3), sc["ric"])
        assert info["triangulated"] >= n - 5 and FR.same_table(tab.download(), twin.download()) is None
        assert tab.download().tobytes() != table
    finally:
        win.set_params(G=(0.0, 0.0, 9.8))                  # the module's handle goes on with the default
        twin.close()
        tab.close()


# ---- slots that are empty or do not exist yet give no factor -------------------------------------------------------------------
def test_fill_passes_none_for_empty_and_missing_slots(pkg, win):
    class Optimizer:
        def __init__(self):
            self.got = {}

        def set_imu(self, j, record=None):
            self.got[j] = record

    class Marginalizer:
        def set_imu(self, sum_dt, residual=None, jacobians=None):
            self.got = (sum_dt, residual, jacobians)

    dt, acc, gyr = R.samples(95, 6, vary=True)
    est = _start(win)
    _both(win, est, 0, dt[:1], acc[:1], gyr[:1])
    _both(win, est, 10, dt[1:], acc[1:], gyr[1:])
    win.slide_old()                                         # slot 9 holds five samples, slot 10 exists and is empty, 1..8 do not exist
    est.slide_old()
    _both(win, est, 3, dt[:2], acc[:2], gyr[:2])
    O, V = Optimizer(), Marginalizer()
    win.fill(O)
    assert sorted(O.got) == list(range(1, R.SLOTS)) and [j for j in O.got if O.got[j] is not None] == [3, 9]
    assert _exists(pkg, win, 10) and win.count(10) == 0 and not _exists(pkg, win, 1)
    for j in (3, 9):
        assert R.same_record(_rec(O.got[j]), est.record(j)) is None
    poses, sbs = np.tile(np.r_[0, 0, 0, 0, 0, 0, 1.0], (R.SLOTS, 1)), np.zeros((R.SLOTS, 9))
    win.fill_marginalizer(V, poses, sbs)                    # slot 1 does not exist
    assert V.got == (0.0, None, None)
    win.slide_old()
    win.slide_old()                                         # slot 1 is the two-sample slot now
    win.fill_marginalizer(V, poses, sbs)
    assert V.got[0] == float(win.record(1)["sum_dt"][0]) > 0 and V.got[1].shape == (15,) and [j.shape for j in V.got[2]] == [(15, 7), (15, 9), (15, 7), (15, 9)]
    for _ in range(8):
        win.slide_old()                                     # slot 1 exists and is empty
    assert win.count(1) == 0
    win.fill_marginalizer(V, poses, sbs)
    assert V.got == (0.0, None, None)


# ---- the C++ mirror -------------------------------------------------------------------------------------------------------
def test_cpp_mirror_equals_the_python_class(pkg, hip, tmp_path):
    """host/lvi_preint_host.hpp beside lvi_win_host.hpp and lvi_marg_host.hpp in a driver of its own, compiled against
    liblvi_hip.so and run once as a child process: the records, preIntegrations[] and imuResidual / imuJacobians of a
    12-image sequence, then a repropagate and a lidarInitialise (refused, then accepted, with a push under the new G), equal the
    Python class's bytes"""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.dirname(pkg.HIP_LIB_PATH)
    exe = tmp_path / "preint_mirror"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(pkg.PKG_DIR, "host"), "-o", str(exe),
                        os.path.join(here, "preint_mirror_driver.cpp"), "-L" + csrc, "-llvi_hip", "-Wl,-rpath," + csrc], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rs = np.random.RandomState(21)
    slides = {10: 2, 11: 1}                                  # image 10: MARGIN_SECOND_NEW, image 11: MARGIN_OLD
    blob, want = np.array([float(CAP), 12.0]).tobytes(), b""
    w = pkg.ImuWindow(hip, max_samples=CAP)
    try:
        frame_count = 0
        for image in range(12):
            n = 1 if image == 0 else int(rs.randint(2, 8))
            dt, acc, gyr = R.samples(500 + image, n, vary=True)
            blob += np.array([float(n), float(slides.get(image, 0))]).tobytes() + np.c_[dt, acc, gyr].tobytes()
            for k in range(n):
                w.process_imu(dt[k], acc[k], gyr[k])
            w.flush(frame_count)
            if image not in slides:
                frame_count += 1
                continue
            pose = np.array([np.r_[rs.normal(0, 1, 3), M.rand_quat(rs, 0.5)] for _ in range(R.SLOTS)])
            sb = np.c_[rs.normal(0, 1, (R.SLOTS, 3)), rs.normal(0, 0.02, (R.SLOTS, 3)), rs.normal(0, 0.002, (R.SLOTS, 3))]
            nav = dict(P=pose[10, :3], R=M.rot(pose[10, 3:]), V=sb[10, :3], Ba=sb[10, 3:6], Bg=sb[10, 6:9])
            blob += pose.tobytes() + sb.tobytes() + np.r_[nav["P"], nav["R"].ravel(), nav["V"], nav["Ba"], nav["Bg"]].tobytes()
            recs = np.zeros(10, pkg.win.IMU_DTYPE)
            for j in range(1, R.SLOTS):
                recs[j - 1] = w.record(j)[0]
            res, J = w.evaluate(1, pose[0], sb[0], pose[1], sb[1])
            want += recs.tobytes() + np.ones(10).tobytes() + np.array([1.0, float(w.record(1)["sum_dt"][0])]).tobytes() + res.tobytes() + \
                np.concatenate([j.ravel() for j in J]).tobytes()
            w.set_nav(**nav)
            w.slide_old() if slides[image] == 1 else w.slide_new()
            want += b"".join(w.record(j).tobytes() for j in range(R.SLOTS))
            n2 = w.nav()
            want += np.r_[n2["P"], n2["R"].ravel(), n2["V"], n2["Ba"], n2["Bg"]].tobytes()
        # after the images: one repropagate of three slots, then lidarInitialise over an empty table, refused and accepted
        Bas, Bgs = rs.normal(0, 0.02, (R.SLOTS, 3)), rs.normal(0, 0.002, (R.SLOTS, 3))
        slots = [2, 5, 10]
        blob += np.r_[float(sum(1 << i for i in slots)), Bas.ravel(), Bgs.ravel()].tobytes()
        w.repropagate(Bas, Bgs, slots)
        records = lambda: b"".join(w.record(j).tobytes() for j in range(R.SLOTS))
        want += records()
        tab = pkg.FeatureTable(hip, max_features=8)
        try:
            frames = [dict(reset_id=3, T=rs.normal(0, 1, 3), R=M.rot(M.rand_quat(rs, 0.5)), V=np.zeros(3), Ba=rs.normal(0, 0.02, 3), Bg=rs.normal(0, 0.002, 3),
                           gravity=9.81) for _ in range(R.SLOTS)]
            d3, a3, g3 = R.samples(600, 3, vary=True)
            blob += np.concatenate([np.array([f[k] for f in frames]).ravel() for k in ("T", "R", "Ba", "Bg")]).tobytes() + \
                np.r_[9.81, np.eye(3).ravel()].tobytes() + np.c_[d3, a3, g3].tobytes()
            bad = [dict(f) for f in frames]
            bad[4]["reset_id"] = -1
            assert w.lidar_initialise(tab, bad) is None
            want += np.array([0.0]).tobytes() + records()
            assert w.lidar_initialise(tab, frames) is not None
            want += np.array([1.0, 0.0, 0.0, 9.81]).tobytes() + records()
            w.push(10, d3, a3, g3)
            n3 = w.nav()
            want += w.record(10).tobytes() + np.r_[n3["P"], n3["R"].ravel(), n3["V"], n3["Ba"], n3["Bg"]].tobytes()
        finally:
            tab.close()
    finally:
        w.close()
    (tmp_path / "in.bin").write_bytes(blob)
    out = subprocess.run(["timeout", "-k", "10", "60", str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = (tmp_path / "out.bin").read_bytes()
    print(f"[preint gpu] C++ mirror: {len(got)} bytes of records, preIntegrations[], imuResidual and imuJacobians")
    assert len(got) == len(want) > (2 * (10 + 11) + 3 * 11 + 1) * 3752 and got == want
