"""CPU tier: the closed-form float64 reference of transformUpdate (tests/update_ref.py) against known answers, then the
ORACLE's tf2 restatement alone against it over the full grid of update_ref.full_grid(): five handles (weight, rotation and z
tolerance), poses on both sides of +-pi/2 and +-pi, hints on, next to and on either side of the 1.4 gate, hints equal to and one
float32 away from the pose's own roll.  tests/test_gpu_update.py runs a thinned grid on the device against the same reference.

Bar: the whole chain runs in doubles and is rounded to float32 once, so |got_k - want_k| <= 1 U with
U = np.spacing(float32(max(|T_k|, |want_k|))), for the components transformUpdate touches (roll, pitch, z); yaw, x and y come
back bit for bit.  No measured constant in it.  Measured: the oracle's worst deviation over the grid is 1.0 U."""
import math

import numpy as np
import pytest

import update_ref as R
from helpers import small_params

PI = math.pi


# ----------------------------------------------------------------------------- update_ref against known answers
def test_blend_moves_the_weighted_share_of_the_short_way():
    imu = dict(imu_available=1, roll=0.5, pitch=-0.4)
    got, taken = R.update_ref([0.1, 0.2, 0.7, 1, 2, 3], imu, 0.25, 1000, 1000)
    assert taken
    assert got[0] == R.f32(R.f32(0.1) + R.f32(0.25) * (R.f32(0.5) - R.f32(0.1)))
    assert got[1] == R.f32(R.f32(0.2) + R.f32(0.25) * (R.f32(-0.4) - R.f32(0.2)))
    assert got[2:] == [R.f32(0.7), 1.0, 2.0, 3.0]
    # the short way round: from 3.0 towards -3.0 is +0.283 through pi, not -6 through zero
    got, _ = R.update_ref([3.0, 0, 0, 0, 0, 0], dict(roll=-3.0, pitch=0.0), 0.5, 1000, 1000)
    assert got[0] == pytest.approx(3.0 + 0.5 * (2 * PI - 6.0), abs=1e-6)
    got, _ = R.update_ref([3.1, 0, 0, 0, 0, 0], dict(roll=-3.1, pitch=0.0), 1.0, 1000, 1000)
    assert got[0] == pytest.approx(-3.1, abs=1e-6)                        # ... and across the seam of atan2


def test_pitch_beyond_half_pi_folds_and_weight_zero_still_wraps():
    got, _ = R.update_ref([4.0, 2.0, 0, 0, 0, 0], dict(roll=4.0, pitch=0.0), 0.0, 1000, 1000)
    assert got[0] == R.f32(4.0 - 2 * PI) and got[1] == R.f32(PI - 2.0)    # getRPY returns the principal values
    got, _ = R.update_ref([0.0, 2.0, 0, 0, 0, 0], dict(roll=0.0, pitch=1.2), 0.5, 1000, 1000)
    assert got[1] == pytest.approx(PI - 1.6, abs=1e-6)                    # half way from 2.0 to 1.2 is 1.6, beyond pi/2: folded
    got, _ = R.update_ref([0.0, -3.0, 0, 0, 0, 0], dict(roll=0.0, pitch=0.2), 0.5, 1000, 1000)
    assert got[1] == pytest.approx(1.4, abs=1e-6)                         # the short way from -3.0 to 0.2 is -3.083 (through -pi): -4.5416 = 1.7416, folded
    got, taken = R.update_ref([4.0, 2.0, 0, 0, 0, 0], None, 0.5, 1000, 1000)
    assert not taken and got[:2] == [4.0, 2.0]                            # no hint: nothing wraps, nothing folds


def test_gate_is_the_promoted_float_against_the_double():
    below = R.f32(1.4)
    assert below < 1.4 < R.nextafter_f32(1.4, 2)                          # float32(1.4) = 1.39999997…
    for p, want in ((below, True), (-below, True), (R.nextafter_f32(1.4, 2), False), (-R.nextafter_f32(1.4, 2), False),
                    (R.nextafter_f32(1.4, 0), True), (1.5, False), (0.0, True)):
        assert R.gate(dict(imu_available=1, roll=0.0, pitch=p)) == want, p
    assert not R.gate(None) and not R.gate(dict(imu_available=0, roll=0.0, pitch=0.0))
    assert R.IMU_PITCH[R.ON_THE_GATE[0]] == below and R.IMU_PITCH[R.ON_THE_GATE[1]] == -below


def test_clamps_are_the_two_comparisons():
    got, _ = R.update_ref([0.7, -0.9, 0.1, 1, 2, 3.0], None, 0.5, 0.5, 0.25)
    assert got == [0.5, -0.5, R.f32(0.1), 1.0, 2.0, 0.25]
    got, _ = R.update_ref([0.7, -0.9, 0.1, 1, 2, -0.2], None, 0.5, 0.0, 0.0)
    assert got[0] == 0 and got[1] == 0 and got[5] == 0
    got, _ = R.update_ref([0.3, -0.2, 0.1, 1, 2, -0.2], dict(roll=0.3, pitch=1.0), 0.5, 0.5, 0.5)
    assert got[0] == R.f32(0.3) and got[1] == R.f32(R.f32(-0.2) + 0.5 * (1.0 - R.f32(-0.2))) and got[5] == R.f32(-0.2)


def test_exclusion_is_the_neighbourhood_of_pi():
    assert R.excluded([0.0, 0.0], dict(roll=PI - 5e-4, pitch=0.0))
    assert R.excluded([0.0, 3.0], dict(roll=0.0, pitch=3.0 - PI + 5e-4))
    assert R.excluded([4.0, 0.0], dict(roll=4.0 - 3 * PI + 5e-4, pitch=0.0))
    assert not R.excluded([0.0, 0.0], dict(roll=PI - 2e-3, pitch=-(PI - 2e-3)))
    assert not R.excluded([0.0, 0.0], None)


def test_the_thinned_grid_keeps_what_it_has_to():
    """what the device tier must not lose (a subset of the full grid, at most about 2 000 calls)"""
    full = {(c.handle, c.i0, c.i1, c.ir, c.ip) for c in R.full_grid()}
    thin = R.thinned_grid()
    keys = [(c.handle, c.i0, c.i1, c.ir, c.ip) for c in thin]
    assert len(set(keys)) == len(keys) and set(keys) <= full and 1000 < len(keys) <= 2000
    for h in range(len(R.HANDLES)):
        mine = [c for c in thin if c.handle == h]
        for ip in range(len(R.IMU_PITCH)):                                # every value of IMU pitch — both signs of float32(1.4) among them — with every T1
            t1 = {c.i1 for c in mine if c.ip == ip}
            want = {i1 for i1 in range(len(R.ANGLES)) if not R.excluded([0.0, R.ANGLES[i1]], dict(roll=0.0, pitch=R.IMU_PITCH[ip]))}
            assert t1 == want and len(want) >= len(R.ANGLES) - 1, (h, ip)
        for ir in R.ROLL_AT_T0:                                           # the hint on and next to the pose's own roll, at every T0
            assert {c.i0 for c in mine if c.ir == ir} == set(range(len(R.ANGLES))), (h, ir)
        for i1 in R.BEYOND_HALF_PI:
            assert sum(c.i1 == i1 for c in mine) >= len(R.IMU_PITCH) - 1, (h, i1)
        assert {(c.i0, c.i1) for c in mine} == {(i0, i1) for i0 in range(len(R.ANGLES)) for i1 in range(len(R.ANGLES))}
    assert len(R.BEYOND_HALF_PI) == 6 and R.HANDLES[-1] == (0.0, 0.0, 0.0)
    # the counts that tests/test_gpu_update.py asserts on the device's gate decisions
    dec = [(c, R.want_of(c)) for c in thin]
    dec = [(c, t) for c, (want, t) in dec if R.gate_decision(c.T, want, c.imu, *R.HANDLES[c.handle]) is not None]
    assert sum(c.ip in R.ON_THE_GATE for c, t in dec) >= 100 and sum(t for c, t in dec) > 300 and sum(not t for c, t in dec) > 100
    for h, (w, rot_tol, z_tol) in enumerate(R.HANDLES):
        if w:
            for ip in R.ON_THE_GATE:
                assert sum(c.handle == h and c.ip == ip and t for c, t in dec) >= 8, (h, ip)


# ----------------------------------------------------------------------------- the oracle over the full grid
@pytest.fixture(scope="module")
def scene():
    return R.far_map_scene()


def check_case(A, T, r, want, label):
    """the four per-case assertions; returns the deviation in U"""
    assert r["status"] == A.LVI_TOO_FEW_CORRESPONDENCES, (label, r["status"])
    assert np.isfinite(r["pose"]).all(), (label, r["pose"])
    dev = max(R.deviation_in_u(T, r["pose"], want))
    assert dev <= 1.0, (label, list(map(float, r["pose"])), want, dev)
    assert R.untouched(T, r["pose"]), (label, r["pose"], T)
    return dev


@pytest.mark.parametrize("h", range(len(R.HANDLES)), ids=[f"w{w:g}_rot{a:g}_z{b:g}" for w, a, b in R.HANDLES])
def test_oracle_meets_the_closed_form_on_the_full_grid(pkg, oracle, scene, h):
    A = pkg._abi
    cases = [c for c in R.full_grid() if c.handle == h]
    assert len(cases) > 4000
    o = pkg.LidarHotpath(oracle, **small_params(**R.handle_params(h)))
    o.map_set(scene["map"], scene["map"])
    worst, taken, decidable = 0.0, 0, 0
    for c in cases:
        want, t = R.want_of(c)
        r = R.run_case(o, scene, c)
        worst = max(worst, check_case(A, c.T, r, want, c))
        taken += t
        d = R.gate_decision(c.T, r["pose"], c.imu, *R.HANDLES[h])       # the gate as the pose shows it, wherever it shows
        assert d is None or d == t, (c, r["pose"], want)
        decidable += d is not None
    o.close()
    print(f"handle {R.HANDLES[h]}: {len(cases)} cases, gate taken {taken} / skipped {len(cases) - taken} ({decidable} decidable from the pose), "
          f"oracle worst {worst:.2f} U")
    assert 0 < taken < len(cases)
    assert (decidable > 0.9 * len(cases)) if R.HANDLES[h][0] and R.HANDLES[h][1] > 100 else (decidable < 0.9 * len(cases))


@pytest.mark.parametrize("imu", [None, dict(imu_available=0, roll=0.9, pitch=-0.7, yaw=0.0)], ids=["no_hint", "hint_not_available"])
def test_oracle_without_a_usable_hint_only_clamps(pkg, oracle, scene, imu):
    A = pkg._abi
    for h in (2, 4):                                                      # the biting and the zero tolerances
        w, rot_tol, z_tol = R.HANDLES[h]
        o = pkg.LidarHotpath(oracle, **small_params(**R.handle_params(h)))
        o.map_set(scene["map"], scene["map"])
        for n, (a, b) in enumerate((i, j) for i in R.ANGLES for j in R.ANGLES):
            T = [R.f32(a), R.f32(b), R.f32(-0.4), R.f32(0.37), R.f32(-1.21), R.f32(R.Z[n % 2])]
            want, taken = R.update_ref(T, imu, w, rot_tol, z_tol)
            assert not taken
            assert want[:2] == [R.clamp(T[0], rot_tol), R.clamp(T[1], rot_tol)]
            r = o.scan_to_map(scene["corner"], scene["surf"], T, imu)
            check_case(A, T, r, want, (h, T))
            assert [float(v) for v in r["pose"][[0, 1, 5]]] == [want[0], want[1], want[5]]          # clamps alone: exact
        o.close()


def test_oracle_soft_outcomes_return_the_guess_unclamped(pkg, oracle, scene):
    """LVI_NO_MAP and LVI_TOO_FEW_FEATURES never reach transformUpdate (mapOptimization.cpp:1317-1320)"""
    A = pkg._abi
    guess = np.array([0.7, -0.9, 0.1, 0.37, -1.21, 3.0], np.float32)
    imu = dict(imu_available=1, roll=0.1, pitch=0.2, yaw=0.0)
    o = pkg.LidarHotpath(oracle, **small_params(icp_max_iters=1, imuRPYWeight=0.5, rotation_tollerance=0.5, z_tollerance=0.5))
    few = scene["surf"][:5]
    for hint in (None, imu):
        r = o.scan_to_map(scene["corner"], scene["surf"], guess, hint)
        assert r["status"] == A.LVI_NO_MAP
        np.testing.assert_array_equal(r["pose"].view(np.uint32), guess.view(np.uint32))
    o.map_set(scene["map"], scene["map"])
    for hint in (None, imu):
        r = o.scan_to_map(few, few, guess, hint)
        assert r["status"] == A.LVI_TOO_FEW_FEATURES
        np.testing.assert_array_equal(r["pose"].view(np.uint32), guess.view(np.uint32))
    r = o.scan_to_map(scene["corner"], scene["surf"], guess, None)       # the same handle does clamp once the gates pass
    assert r["status"] == A.LVI_TOO_FEW_CORRESPONDENCES and r["pose"][5] == 0.5 and r["pose"][0] == 0.5 and r["pose"][1] == -0.5
    o.close()
