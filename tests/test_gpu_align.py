"""GPU tier of the visual-inertial alignment (include/lvi_align.h) against tests/align_ref.py.

The device runs only IEEE + - * / sqrt in the order csrc/lvi_align_math.hpp states, with contraction off, so every comparison
with the float64 reference is equality of bits (np.array_equal: -0.0 == 0.0): the frame records, delta_bg, the five systems,
the five solutions, g, s, the result and the reason.  lvi_align_apply runs on the host with atan2, sin and cos and is held to
the bar of tests/test_align_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import align_ref as R

pytestmark = pytest.mark.gpu

MAXF, MAXS = 66, 48
PRE_FIELDS = ("sum_dt", "delta_p", "delta_q", "delta_v", "linearized_ba", "linearized_bg", "linearized_acc", "linearized_gyr", "jacobian")


@pytest.fixture(scope="module")
def al(pkg, hip):
    a = pkg.ImuAligner(hip, max_frames=MAXF, max_samples=MAXS)
    yield a
    a.close()


def _device_solve(dev, Bgs):
    """a solve on the device with everything the reference is compared on -> the arguments of R.check_solve after sv"""
    Bout, info = dev.solve(Bgs)
    F = len(dev)
    frames = [dev.frame(i) for i in range(F)]
    systems, built = [], 0
    for w in range(R.SYSTEMS):
        try:
            systems.append(dev.last_system(w))
            built += 1
        except Exception as e:
            assert "did not build" in str(e), e                 # LVI_ERR_STATE: check_solve holds the count to the reference's
            break
    x = np.r_[info["x"], np.zeros(3 * F + 4 - len(info["x"]))]
    return info["reason"], info["n_state"], built, info["delta_bg"], Bout, info["s"], info["g_linear"], info["g"], info["min_pivot"], x, frames, systems


def _reference(sc, params, key=None, Bgs=R.BGS0, erase=None):
    ref = R.Aligner(**params)
    R.feed(ref, sc, key)
    if erase is not None:
        ref.erase_through(erase)
    Bout, info = ref.solve(Bgs)
    return ref, dict(Bgs=Bout, info=info, frames=[ref.record(i) for i in range(len(ref.frames))])


def _both(dev, sc, params, name, key=None, Bgs=R.BGS0, erase=None):
    dev.clear()
    dev.set_params(G=params.get("G", R.PARAMS["G"]), TIC=params.get("TIC", R.PARAMS["TIC"]))
    R.feed(dev, sc, key)
    if erase is not None:
        dev.erase_through(erase)
    ref, sv = _reference(sc, params, key, Bgs, erase)
    got = _device_solve(dev, Bgs)
    R.check_solve(name, sv, *got)
    assert bool(sv["info"]["ok"]) == (got[0] == R.OK)
    return ref, sv, got


# ---- shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3, 4, 11, 63, 64, 65, MAXF])
def test_solve_equals_the_reference_bit_for_bit(al, F):
    sc = R.imu_scene(100 + F, F, samples=2 if F > 11 else 4)
    ref, sv, got = _both(al, sc, dict(TIC=tuple(float(t) for t in sc["motion"].tic)), f"F{F}")
    assert sv["info"]["reason"] == (R.SINGULAR if F < 4 else R.OK), R.REASONS[sv["info"]["reason"]]
    assert got[2] == (1 if F < 4 else 5)                      # the linear system is built, and declared singular by count
    if F >= 4:
        assert abs(sv["info"]["s"] - sc["motion"].s) < 0.05 * sc["motion"].s      # the scene's scale, through midpoint integration


def test_samples_per_frame_cross_every_chunk_edge(al):
    counts = [1, 0, 1, 15, 16, 17, 40, 4, 33, 2, 32]
    sc = R.imu_scene(7, len(counts), counts=counts)
    _both(al, sc, dict(TIC=tuple(float(t) for t in sc["motion"].tic)), "counts")
    assert [al.frame(i)["samples"] for i in range(len(counts))] == [0] + counts[1:]
    f = al.frame(6)
    assert np.array_equal(f["dt"], sc["imu"][6][0]) and np.array_equal(f["acc"], sc["imu"][6][1]) and np.array_equal(f["gyr"], sc["imu"][6][2])


def test_a_handle_of_four_frames(pkg, hip):
    small = pkg.ImuAligner(hip, max_frames=4, max_samples=8)
    try:
        sc = R.imu_scene(9, 4)
        _both(small, sc, dict(TIC=tuple(float(t) for t in sc["motion"].tic)), "max_frames 4")
        with pytest.raises(pkg.LviError) as e:
            small.add_frame(200.0, np.zeros(3), np.zeros(3))
        assert e.value.code == pkg._abi.LVI_ERR_CAPACITY
        # erase makes room, and the slots that were freed are used again
        small.erase_through(sc["stamps"][1])
        small.push_imu(*sc["imu"][1])
        small.add_frame(200.0, np.zeros(3), np.zeros(3))
        assert len(small) == 3 and small.frame(2)["samples"] == 4
    finally:
        small.close()


# ---- branches ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.BRANCHES)
def test_branch_scenes(al, name):
    sc, params, key, Bgs = R.branch_scene(name)
    erase = sc["stamps"][2] if name == "erase" else None
    ref, sv, got = _both(al, sc, params, name, key, Bgs, erase)
    want = dict(F2=R.SINGULAR, F3=R.SINGULAR, F4=R.OK, gnorm=R.GRAVITY_NORM, mirror=R.NEGATIVE_SCALE, gz=R.OK, nan=R.SINGULAR, second=R.OK, erase=R.OK, keys=R.OK,
                neg_refined=R.NEGATIVE_SCALE_REFINED)
    if name in want:
        assert got[0] == want[name]
    assert np.all(np.isfinite(np.r_[got[3], np.ravel(got[4]), got[5], got[6], got[7], got[9]])), "a NaN left the call"
    if name == "gz":
        assert R.normalized3(list(got[6])) == [0.0, 0.0, 1.0]                      # TangentBasis's other branch ran on the device
    if name == "second":
        Bout, info = ref.solve(sv["Bgs"])
        sv2 = dict(Bgs=Bout, info=info, frames=[ref.record(i) for i in range(len(ref.frames))])
        R.check_solve("second-2", sv2, *_device_solve(al, sv["Bgs"]))
    if name == "keys":
        assert [al.frame(i)["key"] for i in range(len(al))] == key
        assert np.array_equal(al.key_rotations(), np.array([np.asarray(sc["poses"][i][0]).ravel() for i in range(len(key)) if key[i]]))


def test_too_few(al):
    al.clear()
    Bout, info = al.solve(R.BGS0)
    assert info["reason"] == R.TOO_FEW and not info["ok"] and np.array_equal(Bout, R.BGS0) and not info["x"].any()
    al.push_imu(np.array([0.01]), np.ones((1, 3)), np.zeros((1, 3)))
    al.add_frame(1.0, np.zeros(3), np.zeros(3))
    assert al.solve(R.BGS0)[1]["reason"] == R.TOO_FEW and al.frame(0)["pre"] is None


def test_two_runs_give_the_same_bytes(al):
    sc = R.imu_scene(21, 11, samples=17)
    runs = []
    for _ in range(2):
        al.clear()
        R.feed(al, sc)
        got = _device_solve(al, R.BGS0)
        runs.append(b"".join(np.asarray(t, np.float64).tobytes() for t in (got[3], got[4], [got[5]], got[6], got[7], got[8], got[9]))
                    + b"".join(np.asarray(f["pre"]["jacobian"]).tobytes() for f in got[10][1:]) + b"".join(np.asarray(t).tobytes() for s3 in got[11] for t in s3))
    assert runs[0] == runs[1]


# ---- a frame's preintegration is an lvi_preint slot's -----------------------------------------------------------------------
def test_frame_records_equal_an_imu_window_slot(pkg, hip, al):
    sc = R.imu_scene(31, 6, counts=[1, 17, 16, 5, 33, 1])
    ba, bg = np.array([0.01, -0.02, 0.005]), np.array([1e-3, 2e-3, -1e-3])
    win = pkg.ImuWindow(hip, max_samples=MAXS)
    try:
        al.clear()
        win.set_nav(np.zeros(3), np.eye(3), np.zeros(3), ba, bg)
        for i in range(6):
            al.push_imu(*sc["imu"][i])
            al.add_frame(sc["stamps"][i], ba, bg)
            win.push(i, *sc["imu"][i])
        fields = ("sum_dt", "delta_p", "delta_q", "delta_v", "linearized_ba", "linearized_bg", "jacobian")

        def same(what):
            for i in range(1, 6):
                f, r = al.frame(i)["pre"], win.record(i)
                for k in fields:
                    assert np.array_equal(np.ravel(f[k]), np.ravel(r[k][0])), (what, i, k)
        same("push")
        Bgs, _ = al.solve(np.tile(bg, (11, 1)))
        Bas = np.zeros((11, 3))
        win.repropagate(Bas, np.tile(Bgs[0], (11, 1)), slots=range(1, 6))
        same("repropagate")
    finally:
        win.close()


def test_the_split_into_pushes_does_not_matter(pkg, hip):
    """one frame's 35 samples one at a time, as 1 + 16 + 18 and at once: the same bytes, and the reference's record"""
    dt, acc, gyr = R.PR.samples(79, 36, vary=True, zero_dt_at=9)       # the first sample only sets acc_0 / gyr_0
    ba, bg = np.array([0.01, -0.02, 0.005]), np.array([1e-3, 2e-3, -1e-3])

    def run(dev, cuts):
        dev.push_imu(dt[:1], acc[:1], gyr[:1])
        dev.add_frame(1.0, ba, bg)
        for a, b in zip(cuts[:-1], cuts[1:]):
            dev.push_imu(dt[a:b], acc[a:b], gyr[a:b])
        dev.add_frame(2.0, ba, bg)

    results = {}
    for name, cuts in (("one at a time", list(range(1, 37))), ("1, 16, 18", [1, 2, 18, 36]), ("at once", [1, 36])):
        dev = pkg.ImuAligner(hip, max_frames=4, max_samples=64)
        try:
            run(dev, cuts)
            f = dev.frame(1)
        finally:
            dev.close()
        assert f["samples"] == 35 and sorted(f["pre"]) == sorted(PRE_FIELDS)
        results[name] = f
    ref = R.Aligner(max_frames=4, max_samples=64)
    run(ref, [1, 36])
    want = ref.record(1)
    once = results["at once"]
    for name, f in results.items():
        for k in PRE_FIELDS:
            assert np.asarray(f["pre"][k], np.float64).tobytes() == np.asarray(once["pre"][k], np.float64).tobytes(), (name, k)
            assert np.array_equal(np.ravel(f["pre"][k]), np.ravel(want["pre"][k])), (name, k)
        for k, v in (("dt", dt), ("acc", acc), ("gyr", gyr)):
            assert f[k].tobytes() == once[k].tobytes() and f[k].tobytes() == np.ascontiguousarray(v[1:]).tobytes(), (name, k)


# ---- errors leave the state as it was -----------------------------------------------------------------------------------
def test_errors_leave_the_state_unchanged(pkg, hip, al):
    E = pkg._abi
    sc = R.imu_scene(41, 8)
    params = dict(TIC=tuple(float(t) for t in sc["motion"].tic))
    ref, sv = _reference(sc, params)
    al.clear()
    al.set_params(G=R.PARAMS["G"], TIC=params["TIC"])
    R.feed(al, sc)
    d = lambda a: a.ctypes.data_as(pkg.align._P(pkg.align._f64))
    z3, info, buf = np.zeros(3), pkg.align.AlignInfo(), np.zeros(64)
    B = R.BGS0.copy()
    dll, h = al.lib.dll, al._h
    small = pkg.ImuAligner(hip, max_frames=2, max_samples=4)
    try:
        for k in range(2):
            small.push_imu(np.array([0.01]), np.ones((1, 3)), np.zeros((1, 3)))
            small.add_frame(1.0 + k, z3, z3)
        assert dll.lvi_align_add_frame(small._h, 5.0, d(z3), d(z3)) == E.LVI_ERR_CAPACITY
        assert dll.lvi_align_push_imu(small._h, 5, d(np.full(5, 0.01)), d(np.ones((5, 3))), d(np.zeros((5, 3)))) == E.LVI_ERR_CAPACITY
        assert len(small) == 2 and small.frame(1)["samples"] == 1
    finally:
        small.close()
    assert dll.lvi_align_add_frame(h, sc["stamps"][-1], d(z3), d(z3)) == E.LVI_ERR_INVALID_ARG          # a stamp out of order
    assert dll.lvi_align_add_frame(h, sc["stamps"][0] - 1.0, d(z3), d(z3)) == E.LVI_ERR_INVALID_ARG
    assert dll.lvi_align_erase_through(h, 12345.0) == E.LVI_ERR_STATE                                   # an unknown t0
    assert dll.lvi_align_set_pose(h, 12345.0, d(np.eye(3)), d(z3), 1) == E.LVI_ERR_STATE
    assert dll.lvi_align_solve(h, None, d(z3), d(buf), 64, pkg.align.C.byref(info)) == E.LVI_ERR_INVALID_ARG      # a NULL pointer
    assert dll.lvi_align_solve(h, d(B), d(z3), None, 64, pkg.align.C.byref(info)) == E.LVI_ERR_INVALID_ARG
    assert dll.lvi_align_push_imu(h, 2, None, None, None) == E.LVI_ERR_INVALID_ARG
    assert dll.lvi_align_solve(h, d(B), d(z3), d(buf), 3 * 8 + 3, pkg.align.C.byref(info)) == E.LVI_ERR_CAPACITY    # cap too small
    bad = np.full((1, 3), np.nan)
    assert dll.lvi_align_push_imu(h, 1, d(np.array([0.01])), d(bad), d(np.zeros((1, 3)))) == E.LVI_ERR_INVALID_ARG
    assert np.array_equal(B, R.BGS0) and len(al) == 8
    with pytest.raises(pkg.LviError) as e:
        al.last_system(0)                                                                               # no solve yet on this state
    assert e.value.code == E.LVI_ERR_STATE
    R.check_solve("after the errors", sv, *_device_solve(al, R.BGS0))
    n = pkg.align._i32(0)
    assert dll.lvi_align_last_system(h, 0, pkg.align.C.byref(n), d(buf), None, None, 64) == E.LVI_ERR_CAPACITY
    assert dll.lvi_align_last_system(h, 5, pkg.align.C.byref(n), None, None, None, 0) == E.LVI_ERR_INVALID_ARG


def test_excitation(al):
    sc = R.imu_scene(51, 7)
    ref = R.Aligner()
    al.clear()
    R.feed(al, sc)
    R.feed(ref, sc)
    assert al.excitation() == ref.excitation()


# ---- the C++ mirror -----------------------------------------------------------------------------------------------------
def test_cpp_mirror_equals_the_python_class(pkg, hip, al, tmp_path):
    """lvi_host::ImageFrames and lvi_host::VisualIMUAlignment through a small driver"""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.dirname(pkg.HIP_LIB_PATH)
    exe = tmp_path / "align_mirror"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(pkg.PKG_DIR, "host"), "-o", str(exe),
                        os.path.join(here, "align_mirror_driver.cpp"), "-L" + csrc, "-llvi_hip", "-Wl,-rpath," + csrc], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    sc = R.imu_scene(61, 9, counts=[1, 4, 17, 3, 16, 2, 5, 1, 4])
    tic = tuple(float(t) for t in sc["motion"].tic)
    key = [i % 2 == 0 for i in range(9)]
    v = [float(MAXF), float(MAXS), *tic, *R.PARAMS["G"], *R.BGS0.ravel(), 9.0]
    for i in range(9):
        dt, acc, gyr = sc["imu"][i]
        v += [sc["stamps"][i], float(len(dt)), *np.c_[dt, acc, gyr].ravel()]
    for i in range(9):
        v += [*np.asarray(sc["poses"][i][0]).ravel(), *sc["poses"][i][1], float(key[i])]
    (tmp_path / "in.bin").write_bytes(np.array(v, np.float64).tobytes())
    out = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.float64)
    al.clear()
    al.set_params(G=R.PARAMS["G"], TIC=tic)
    R.feed(al, sc, key)
    var = al.excitation()
    Bout, info = al.solve(R.BGS0)
    want = np.r_[float(info["ok"]), info["reason"], info["n_state"], info["frames"], var, Bout.ravel(), info["g"], info["delta_bg"], info["s"], info["min_pivot"], info["x"]]
    assert info["ok"] and np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ---- one chain: ImuWindow and ImuAligner side by side ---------------------------------------------------------------------
def _quat(Rm):
    q = R.rot_to_quat([float(t) for t in np.asarray(Rm).ravel()])
    return np.array(q) / np.linalg.norm(q)


def test_one_chain_aligned_states_fit_the_imu_factors(pkg, hip, al):
    """the scene's IMU into an ImuWindow and an ImuAligner, solve, lvi_preint_repropagate with the new Bgs, apply: the position and
    velocity rows of every one of the ten IMU factors are smaller at the aligned states than at the unaligned ones"""
    sc = R.imu_scene(71, 11, samples=20)
    m = sc["motion"]
    tic = tuple(float(t) for t in m.tic)
    win = pkg.ImuWindow(hip, max_samples=MAXS)
    try:
        al.clear()
        al.set_params(G=R.PARAMS["G"], TIC=tic)
        for i in range(11):
            win.push(i, *sc["imu"][i])
            al.push_imu(*sc["imu"][i])
            al.add_frame(sc["stamps"][i], np.zeros(3), np.zeros(3))
        for i in range(11):
            al.set_pose(sc["stamps"][i], sc["poses"][i][0], sc["poses"][i][1], True)
        Bgs, info = al.solve(np.zeros((11, 3)))
        assert info["ok"]
        win.repropagate(np.zeros((11, 3)), Bgs)
        T, Rm = np.array([p[1] for p in sc["poses"]]), np.array([p[0] for p in sc["poses"]])
        Ps, Rs, Vs, g, rot, flags = al.apply(T, Rm, info["x"], info["g"])
        assert flags == 0 and abs(g[0]) < 1e-12 and abs(g[1]) < 1e-12 and abs(g[2] - 9.8) < 1e-9
        assert abs(info["s"] - m.s) < 1e-3 * m.s and np.abs(Vs[0] - rot @ m.R_c0_w @ m.pos(0.0, 1)).max() < 1e-2

        def rows(P, Rr, V, G):
            win.set_params(G=G)
            out = []
            for j in range(1, 11):
                r, _ = win.evaluate(j, np.r_[P[j - 1], _quat(Rr[j - 1])], np.r_[V[j - 1], np.zeros(3), Bgs[j - 1]], np.r_[P[j], _quat(Rr[j])],
                                    np.r_[V[j], np.zeros(3), Bgs[j]])
                out.append((np.linalg.norm(r[0:3]), np.linalg.norm(r[6:9])))
            return np.array(out)
        before = rows(T, Rm, np.zeros((11, 3)), R.PARAMS["G"])
        after = rows(Ps, Rs, Vs, tuple(g))
        print("[align chain] position rows before %.3g..%.3g after %.3g..%.3g; velocity rows before %.3g..%.3g after %.3g..%.3g" %
              (before[:, 0].min(), before[:, 0].max(), after[:, 0].min(), after[:, 0].max(), before[:, 1].min(), before[:, 1].max(), after[:, 1].min(),
               after[:, 1].max()))
        assert np.all(after < before), (before, after)
    finally:
        win.close()
