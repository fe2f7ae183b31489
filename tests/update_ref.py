"""A closed-form float64 reference of transformUpdate (mapOptimization.cpp:1345-1375): the roll / pitch blend towards the IMU
hint, its |imu_pitch_init| < 1.4 gate and the three clamps of constraintTransformation.

The reference slerps two tf2 quaternions about ONE axis (roll alone, then pitch alone) and reads the angle back with getRPY.
For two rotations about one axis the slerp is linear interpolation of the angle along the short way, so the whole of it is

    wrap(x)  = atan2(sin x, cos x)
    roll'    = f32( wrap( T0 + w * wrap(roll_imu  - T0) ) )
    pitch'   = f32( asin(sin( T1 + w * wrap(pitch_imu - T1) )) )          # getRPY folds a pitch beyond +-pi/2

with no quaternion in sight: a model that can judge the oracle's tf2 restatement and the device's alike.  Python floats only;
every float32 input is widened first (float(np.float32(v))), every float32 result is rounded once.

The form holds while |wrap(imu - T)| keeps away from pi: at exactly pi the direction of the slerp is a rounding accident in
the reference itself.  excluded() names those cases; the grids leave them out.

Also here, because both tiers share them: the grid of cases, its thinned form for the device, the far-map scene that makes
scan_to_map return transformUpdate(guess) for any float32 guess, and the 1 U comparison."""
import math
from collections import namedtuple

import numpy as np

PI = math.pi
NEAR_PI = 1e-3


def f32(v):
    """the float32 nearest to v, as a Python float"""
    return float(np.float32(v))


def nextafter_f32(v, towards):
    return float(np.nextafter(np.float32(v), np.float32(towards)))


def wrap(x):
    return math.atan2(math.sin(x), math.cos(x))


def clamp(v, limit):
    """constraintTransformation (:1377-1385): the reference's two comparisons, on float32 values"""
    if v < -limit:
        v = -limit
    if v > limit:
        v = limit
    return v


def gate(imu):
    """does transformUpdate blend?  `std::abs(float) < 1.4`: the float is promoted, the literal is a double.
    (Python floats on purpose: NumPy 2 demotes the 1.4 of `np.float32(p) < 1.4` to float32 and then float32(1.4) < 1.4 is False.)"""
    if imu is None or int(imu.get("imu_available", 1)) == 0:
        return False
    return abs(f32(imu.get("pitch", 0.0))) < 1.4


def excluded(T, imu):
    """is the roll or the pitch hint within NEAR_PI of the opposite direction of the pose's?"""
    if imu is None:
        return False
    return any(PI - abs(wrap(f32(imu[k]) - f32(t))) < NEAR_PI for k, t in (("roll", T[0]), ("pitch", T[1])))


def update_ref(T, imu, w, rot_tol, z_tol, force_gate=None):
    """transformUpdate of the float32 pose T = [roll, pitch, yaw, x, y, z] -> (six Python floats holding float32 values, gate taken).
    force_gate = True / False: what a library that took / skipped the blend regardless of the hint's pitch would return."""
    T = [f32(v) for v in T]
    w, rot_tol, z_tol = f32(w), f32(rot_tol), f32(z_tol)
    roll, pitch = T[0], T[1]
    taken = gate(imu) if force_gate is None else bool(force_gate)
    if taken:
        roll = f32(wrap(T[0] + w * wrap(f32(imu.get("roll", 0.0)) - T[0])))
        pitch = f32(math.asin(math.sin(T[1] + w * wrap(f32(imu.get("pitch", 0.0)) - T[1]))))
    return [clamp(roll, rot_tol), clamp(pitch, rot_tol), T[2], T[3], T[4], clamp(T[5], z_tol)], taken


def deviation_in_u(T, got, want):
    """|got_k - want_k| in units of U = the float32 spacing at max(|T_k|, |want_k|), for the components transformUpdate touches
    (0, 1, 5).  The chain runs in doubles and is rounded once, so the bar is 1.  +0 and -0 are the same value; a NaN is inf."""
    out = []
    for k in (0, 1, 5):
        g = float(got[k])
        if not math.isfinite(g):
            out.append(math.inf)
            continue
        u = float(np.spacing(np.float32(max(abs(f32(T[k])), abs(want[k])))))
        out.append(abs(g - want[k]) / u)
    return out


def gate_decision(T, got, imu, w, rot_tol, z_tol):
    """Which way did the library that returned `got` decide the gate?  Read off roll and pitch: True (blended), False (did not),
    or None where the two outcomes lie within 4 U of each other after the clamps (w = 0 on a pose inside the principal ranges,
    a hint on the pose itself, a clamp that swallows the difference) and so cannot be told apart at the 1 U bar."""
    yes, _ = update_ref(T, imu, w, rot_tol, z_tol, force_gate=True)
    no, _ = update_ref(T, imu, w, rot_tol, z_tol, force_gate=False)
    sep = max(abs(yes[k] - no[k]) / float(np.spacing(np.float32(max(abs(yes[k]), abs(no[k]), 1e-30)))) for k in (0, 1))
    if sep < 4.0:
        return None
    return max(abs(float(got[k]) - yes[k]) for k in (0, 1)) < max(abs(float(got[k]) - no[k]) for k in (0, 1))


def untouched(T, got):
    """components 2, 3, 4 (yaw, x, y) come back bit for bit"""
    a = np.asarray([T[2], T[3], T[4]], np.float32).view(np.uint32)
    b = np.asarray([got[2], got[3], got[4]], np.float32).view(np.uint32)
    return bool((a == b).all())


# ----------------------------------------------------------------------------- the cases
# (imuRPYWeight, rotation_tollerance, z_tollerance) of the five handles
HANDLES = ((0.01, 1000.0, 1000.0), (0.1, 1000.0, 1000.0), (0.5, 0.5, 0.5), (1.0, 1000.0, 1000.0), (0.0, 0.0, 0.0))
ANGLES = (0.0, 1e-7, 0.3, -1.0, PI / 2 - 1e-3, -(PI / 2 + 1e-3), 2.0, -3.0, PI - 1e-3, 4.0, -6.5)          # T0 and T1
BEYOND_HALF_PI = tuple(i for i, a in enumerate(ANGLES) if abs(a) > PI / 2)
IMU_ROLL = (0.1, -2.5, 3.1, "T0", "next")                                                                  # "T0": the pose's own roll; "next": one float32 above it
ROLL_AT_T0 = (3, 4)
IMU_PITCH = (0.0, 0.2, -1.39, f32(1.4), -f32(1.4), nextafter_f32(1.4, 2), nextafter_f32(1.4, 0), 1.5)
ON_THE_GATE = (3, 4)                                                                                       # +-float32(1.4) = 1.39999997…: below the double 1.4
Z = (3.0, -0.2)

Case = namedtuple("Case", "handle T imu i0 i1 ir ip")


def _case(h, i0, i1, ir, ip, n):
    T0, T1 = f32(ANGLES[i0]), f32(ANGLES[i1])
    r = IMU_ROLL[ir]
    roll = T0 if r == "T0" else nextafter_f32(T0, 100) if r == "next" else f32(r)
    T = [T0, T1, f32(0.1 * (n % 7 - 3)), f32(0.37), f32(-1.21), f32(Z[n % 2])]
    return Case(h, T, dict(imu_available=1, roll=roll, pitch=IMU_PITCH[ip], yaw=0.0), i0, i1, ir, ip)


def full_grid():
    """every handle x T0 x T1 x IMU roll x IMU pitch, the cases next to pi left out"""
    out = []
    for h in range(len(HANDLES)):
        n = 0
        for i0 in range(len(ANGLES)):
            for i1 in range(len(ANGLES)):
                for ir in range(len(IMU_ROLL)):
                    for ip in range(len(IMU_PITCH)):
                        c = _case(h, i0, i1, ir, ip, n)
                        n += 1
                        if not excluded(c.T, c.imu):
                            out.append(c)
    return out


def thinned_grid():
    """the grid thinned for the device, on every handle: every T1 with every IMU pitch, every T0 with every IMU roll and every
    (T0, T1) pair, the remaining two indices cycling.  Where the cycled partner lands on a case next to pi the next one is taken."""
    n0, nr, np_ = len(ANGLES), len(IMU_ROLL), len(IMU_PITCH)
    out, seen = [], set()

    def add(h, i0, i1, ir, ip, free):
        for step in range(max(n0, nr, np_)):
            j = dict(i0=i0, i1=i1, ir=ir, ip=ip)
            for name in free:
                j[name] = (j[name] + step) % dict(i0=n0, i1=n0, ir=nr, ip=np_)[name]
            key = (h, j["i0"], j["i1"], j["ir"], j["ip"])
            c = _case(h, j["i0"], j["i1"], j["ir"], j["ip"], len(out))
            if excluded(c.T, c.imu):
                continue
            if key not in seen:
                seen.add(key)
                out.append(c)
            return                                                     # (falls through when the fixed pair itself is next to pi)

    for h in range(len(HANDLES)):
        for i1 in range(n0):
            for ip in range(np_):
                add(h, (i1 + 2 * ip + h) % n0, i1, (i1 + ip) % nr, ip, ("i0", "ir"))
        for i0 in range(n0):
            for ir in range(nr):
                add(h, i0, (i0 + 3 * ir + h) % n0, ir, (i0 + ir) % np_, ("i1", "ip"))
        for i0 in range(n0):
            for i1 in range(n0):
                add(h, i0, i1, (i0 + i1) % nr, (i0 + 2 * i1 + h) % np_, ("ir", "ip"))
    return out


def handle_params(h, **kw):
    w, rot_tol, z_tol = HANDLES[h]
    d = dict(icp_max_iters=1, imuRPYWeight=w, rotation_tollerance=rot_tol, z_tollerance=z_tol)
    d.update(kw)
    return d


def want_of(c):
    w, rot_tol, z_tol = HANDLES[c.handle]
    return update_ref(c.T, c.imu, w, rot_tol, z_tol)


# ----------------------------------------------------------------------------- reaching transformUpdate with a chosen pose
def far_map_scene():
    """a scan that passes the feature-count gates and a map some 500 m away from it: no iteration selects 50 rows, the pose
    never moves, the status is LVI_TOO_FEW_CORRESPONDENCES — and transformUpdate is still applied, to the guess itself
    (mapOptimization.cpp:1317-1341).  Scan: a 12 x 12 x 2 lattice, 1 m apart (one point per voxel of either leaf size)."""
    g = np.arange(12, dtype=np.float32) - 6 + 0.25
    x, y, z = np.meshgrid(g, g, np.array([0.25, 1.25], np.float32), indexing="ij")
    surf = np.stack([x.ravel(), y.ravel(), z.ravel(), np.zeros(x.size, np.float32)], axis=1).astype(np.float32)
    rng = np.random.default_rng(1345)
    far = np.zeros((400, 4), np.float32)
    far[:, :3] = rng.uniform(-5, 5, (400, 3)) + [500, 0, 0]
    return dict(corner=np.ascontiguousarray(surf[::5]), surf=surf, map=far)


def run_case(h, scene, c):
    return h.scan_to_map(scene["corner"], scene["surf"], c.T, c.imu)
