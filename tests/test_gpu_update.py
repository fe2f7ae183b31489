"""GPU tier (-m gpu): what happens after the last row of LVI_DBG_ICP_POSE_TRACE — transformUpdate on the device
(icp_finish_body in csrc/lvi_icp.hip: the roll / pitch slerp towards the IMU hint, its |imu_pitch_init| < 1.4 gate, the clamps
of constraintTransformation, the 32-byte pose record) against the closed-form float64 reference of tests/update_ref.py.

The HIP library is judged by the closed form, never by the oracle; the oracle rides along so that the printed lines show both
worst deviations (its own full-grid check is tests/test_update_ref.py).  Bar: |got_k - want_k| <= 1 U, U = the float32 spacing
at max(|T_k|, |want_k|) — doubles throughout, rounded once — for roll, pitch and z; yaw, x and y bit for bit.

A map some 500 m from the scan makes scan_to_map return transformUpdate(guess) for any float32 guess (update_ref.far_map_scene);
where the loop did run, the pre-update pose is the last row of the trace on both libraries."""
import ctypes as C

import numpy as np
import pytest

import update_ref as R
from helpers import make_small_scene, small_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def far():
    return R.far_map_scene()


@pytest.fixture(scope="module")
def grid_runs(pkg, oracle, hip, far):
    """the thinned grid on both libraries, computed once: [(case, want, gate taken, oracle result, hip result)]"""
    cases = R.thinned_grid()
    assert len(cases) <= 2000
    out = []
    for h in range(len(R.HANDLES)):
        o = pkg.LidarHotpath(oracle, **small_params(**R.handle_params(h)))
        g = pkg.LidarHotpath(hip, **small_params(**R.handle_params(h)))
        for x in (o, g):
            x.map_set(far["map"], far["map"])
        for c in cases:
            if c.handle == h:
                want, taken = R.want_of(c)
                out.append((c, want, taken, R.run_case(o, far, c), R.run_case(g, far, c)))
        o.close(); g.close()
    return out


# ----------------------------------------------------------------------------- (a)
def test_device_meets_the_closed_form(pkg, grid_runs):
    A = pkg._abi
    worst = {"oracle": 0.0, "hip": 0.0}
    where = {}
    bad = []
    for c, want, taken, ro, rg in grid_runs:
        for name, r in (("oracle", ro), ("hip", rg)):
            dev = max(R.deviation_in_u(c.T, r["pose"], want))
            if dev > worst[name]:
                worst[name], where[name] = dev, c
        ok = (rg["status"] == A.LVI_TOO_FEW_CORRESPONDENCES and bool(np.isfinite(rg["pose"]).all())
              and max(R.deviation_in_u(c.T, rg["pose"], want)) <= 1.0 and R.untouched(c.T, rg["pose"]))
        if not ok:
            bad.append((c, want, [float(v) for v in rg["pose"]], rg["status"]))
    print(f"transformUpdate, {len(grid_runs)} cases: worst deviation from the closed form  HIP {worst['hip']:.2f} U  oracle {worst['oracle']:.2f} U")
    for name in worst:
        print(f"  {name} worst at {where.get(name)}")
    assert not bad, (len(bad), bad[:5])


# ----------------------------------------------------------------------------- (b)
def test_gate_decision_is_the_reference_s(grid_runs):
    """Read off the pose (update_ref.gate_decision): wherever taking and skipping the blend differ by 4 U or more, the device
    decides as the closed form does.  The cases on the gate itself — IMU pitch = +-float32(1.4), which the reference promotes
    to a double just below 1.4 and therefore blends — are among them on every handle with w != 0."""
    count = {name: {True: 0, False: 0} for name in ("closed form", "hip", "oracle")}
    wrong, on_gate = [], 0
    for c, want, taken, ro, rg in grid_runs:
        args = (c.imu,) + R.HANDLES[c.handle]
        if R.gate_decision(c.T, want, *args) is None:
            continue
        count["closed form"][taken] += 1
        on_gate += c.ip in R.ON_THE_GATE
        for name, r in (("oracle", ro), ("hip", rg)):
            d = R.gate_decision(c.T, r["pose"], *args)
            count[name][d] += 1
            if name == "hip" and d != taken:
                wrong.append((c, "the reference blends" if taken else "the reference does not blend", [float(v) for v in r["pose"]]))
    show = {k: f"taken {v[True]} / skipped {v[False]}" for k, v in count.items()}
    print(f"gate decisions on {sum(count['closed form'].values())} decidable cases ({on_gate} of them with IMU pitch = +-float32(1.4)): {show}")
    assert on_gate >= 100 and count["closed form"][True] > 300 and count["closed form"][False] > 100
    assert not wrong, (len(wrong), wrong[:4])
    assert count["hip"] == count["closed form"]


# ----------------------------------------------------------------------------- (c)
def test_finish_step_applies_the_update_once(pkg, oracle, hip, far):
    """20 iterations with the reference's break rule: the device enqueues the loop in chunks and runs the finish kernel after
    each (lvi_icp.hip, icp_finish_body works on copies).  w = 0.5 and a 0.4 rad offset: once is 0.2 of the way, twice 0.3."""
    A = pkg._abi
    T = [R.f32(v) for v in (0.3, -0.25, 0.4, 0.37, -1.21, 3.0)]
    imu = dict(imu_available=1, roll=T[0] + 0.4, pitch=T[1] - 0.4, yaw=0.0)
    want, taken = R.update_ref(T, imu, 0.5, 1000.0, 1000.0)
    assert taken and abs(want[0] - (T[0] + 0.2)) < 1e-6 and abs(want[1] - (T[1] - 0.2)) < 1e-6
    for lib in (oracle, hip):
        h = pkg.LidarHotpath(lib, **small_params(imuRPYWeight=0.5))
        assert h.params.icp_max_iters == 20 and h.params.icp_disable_break == 0
        h.map_set(far["map"], far["map"])
        r = h.scan_to_map(far["corner"], far["surf"], T, imu)
        h.close()
        assert r["status"] == A.LVI_TOO_FEW_CORRESPONDENCES and r["iters"] == 20
        assert max(R.deviation_in_u(T, r["pose"], want)) <= 1.0 and R.untouched(T, r["pose"]), (r["pose"], want)


# ----------------------------------------------------------------------------- (d)
@pytest.fixture(scope="module")
def scene(pkg, oracle):
    return make_small_scene(pkg, oracle)


def _staged(pkg, lib, scene, **kw):
    h = pkg.LidarHotpath(lib, **small_params(**kw))
    h.map_set(scene["map_corner"], scene["map_surf"])
    h.scan_upload(scene["scan"]); h.scan_organize(); h.scan_extract(); h.scan_downsample()
    return h


BITING = dict(rotation_tollerance=0.004, z_tollerance=0.25)


def test_update_of_the_loop_that_did_run(pkg, oracle, hip, scene):
    """pose == update_ref(trace[-1]) where Gauss-Newton moved the pose, with tolerances far away and with tolerances that bite"""
    A = pkg._abi
    for name, lib in (("oracle", oracle), ("hip", hip)):
        for tol in (dict(rotation_tollerance=1000.0, z_tollerance=1000.0), BITING):
            h = _staged(pkg, lib, scene, imuRPYWeight=0.5, **tol)
            solved = h.scan_match(scene["guess"])
            assert solved["status"] == A.LVI_OK
            pre = h.debug_get(A.DBG_ICP_POSE_TRACE, np.float32).reshape(-1, 6)[-1]
            imu = dict(imu_available=1, roll=float(pre[0]) + 0.1, pitch=float(pre[1]) - 0.2, yaw=0.0)
            r = h.scan_match(scene["guess"], imu)
            trace = h.debug_get(A.DBG_ICP_POSE_TRACE, np.float32).reshape(-1, 6)
            h.close()
            assert r["status"] == A.LVI_OK and len(trace) == r["iters"] + 1
            T = [float(v) for v in trace[-1]]
            if tol is BITING:                              # precondition: the clamps are below what the loop arrived at
                assert tol["rotation_tollerance"] < min(abs(T[0]), abs(T[1])) and tol["z_tollerance"] < abs(T[5]), T
            want, taken = R.update_ref(T, imu, 0.5, tol["rotation_tollerance"], tol["z_tollerance"])
            dev = R.deviation_in_u(T, r["pose"], want)
            print(f"{name} tolerances {tol}: trace[-1] {T[:2] + T[5:]} -> {[float(r['pose'][k]) for k in (0, 1, 5)]}, {max(dev):.2f} U from the closed form")
            assert taken and max(dev) <= 1.0 and R.untouched(T, r["pose"]), (name, tol, r["pose"], want)
            if tol is BITING:
                assert [abs(float(r["pose"][k])) for k in (0, 1, 5)] == [R.f32(0.004), R.f32(0.004), 0.25]
            else:
                assert abs(want[0] - T[0] - 0.05) < 1e-6 and abs(want[1] - T[1] + 0.1) < 1e-6


# ----------------------------------------------------------------------------- (e)
def test_soft_outcomes_leave_the_guess_bit_for_bit(pkg, oracle, hip, far):
    """LVI_NO_MAP and LVI_TOO_FEW_FEATURES never reach transformUpdate: biting tolerances and a hint change nothing"""
    A = pkg._abi
    guess = np.array([0.7, -0.9, 0.1, 0.37, -1.21, 3.0], np.float32)
    imu = dict(imu_available=1, roll=0.1, pitch=0.2, yaw=0.0)
    few = far["surf"][:5]
    for lib in (oracle, hip):
        h = pkg.LidarHotpath(lib, **small_params(icp_max_iters=1, imuRPYWeight=0.5, rotation_tollerance=0.5, z_tollerance=0.5))
        for hint in (None, imu):
            r = h.scan_to_map(far["corner"], far["surf"], guess, hint)
            assert r["status"] == A.LVI_NO_MAP
            np.testing.assert_array_equal(r["pose"].view(np.uint32), guess.view(np.uint32))
        h.map_set(far["map"], far["map"])
        for hint in (None, imu):
            r = h.scan_to_map(few, few, guess, hint)
            assert r["status"] == A.LVI_TOO_FEW_FEATURES
            np.testing.assert_array_equal(r["pose"].view(np.uint32), guess.view(np.uint32))
        r = h.scan_to_map(far["corner"], far["surf"], guess, None)       # the same handle does clamp once the gates pass
        assert r["status"] == A.LVI_TOO_FEW_CORRESPONDENCES and [float(v) for v in r["pose"][[0, 1, 5]]] == [0.5, -0.5, 0.5]
        h.close()


# ----------------------------------------------------------------------------- (f)
def test_records_carry_the_clamped_pose(pkg, hip, scene):
    """the 32-byte record of lvi_scan_match_async and of a two-slot batch: pose bits and status of the synchronous
    lvi_scan_match of the same handle / the same scans, with tolerances that bite and no hint"""
    A = pkg._abi
    S = pkg.synth
    rt = C.CDLL("libamdhip64.so.7")                          # the runtime liblvi_hip.so is linked against
    rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipFree.argtypes = [C.c_void_p]
    d_rec = C.c_void_p()
    assert rt.hipMalloc(C.byref(d_rec), 32) == 0
    g = _staged(pkg, hip, scene, **BITING)
    sync = g.scan_match(scene["guess"])
    assert sync["status"] == A.LVI_OK
    pre = g.debug_get(A.DBG_ICP_POSE_TRACE, np.float32).reshape(-1, 6)[-1]
    assert BITING["rotation_tollerance"] < min(abs(pre[0]), abs(pre[1])) and BITING["z_tollerance"] < abs(pre[5])
    assert [abs(float(sync["pose"][k])) for k in (0, 1, 5)] == [R.f32(0.004), R.f32(0.004), 0.25]
    zero = np.zeros(8, np.float32)
    assert rt.hipMemcpy(d_rec, zero.ctypes.data, 32, 1) == 0
    g.scan_match_async(scene["guess"], d_rec.value)
    g.sync()
    rec = np.zeros(8, np.float32)
    assert rt.hipMemcpy(rec.ctypes.data, d_rec, 32, 2) == 0
    rt.hipFree(d_rec)
    np.testing.assert_array_equal(rec[:6].view(np.uint32), sync["pose"].view(np.uint32))
    assert int(rec[6:7].view(np.int32)[0]) == sync["status"] and int(rec[7:8].view(np.int32)[0]) == sync["iters"]
    own = g.get_pose_record()
    np.testing.assert_array_equal(own["pose"].view(np.uint32), sync["pose"].view(np.uint32))
    assert own["status"] == sync["status"]
    # ---- two slots
    pose2 = S.loop_pose(0.97, 0.01, -0.02)
    scans = [scene["scan"], S.make_scan(12000, pose2, 901)]
    guesses = np.stack([scene["guess"], S.perturbed_guess(pose2, 21)])
    g.scan_upload(scans[1]); g.scan_organize(); g.scan_extract(); g.scan_downsample()
    singles = [sync, g.scan_match(guesses[1])]
    g.close()
    assert singles[1]["status"] == A.LVI_OK and abs(float(singles[1]["pose"][5])) == 0.25
    b = pkg.LidarHotpath(hip, **small_params(batch_scans=2, **BITING))
    b.map_upload(scene["map_corner"], scene["map_surf"]); b.map_build()
    b.batch_upload(scans)
    b.batch_run(guesses, 0, rebuild_map=False)
    recs = b.batch_get_records(2)
    b.close()
    for k in range(2):
        np.testing.assert_array_equal(recs[k, :6].view(np.uint32), singles[k]["pose"].view(np.uint32), err_msg=f"slot {k}")
        assert int(recs[k, 6:7].view(np.int32)[0]) == singles[k]["status"] and int(recs[k, 7:8].view(np.int32)[0]) == singles[k]["iters"]
