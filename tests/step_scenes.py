"""Deterministic feature-level scenes for the end of a Gauss-Newton iteration (tests/step_ref.py): clouds that go straight into
LidarHotpath.map_set / scan_to_map (no raw scan, no organise / extract stage), about 1 200 scan points each.

Geometry.  Points lie on lattices of one point per voxel (leaf 0.2 m for corners, 0.4 m for surfaces) with a jitter below
0.3 leaf inside each face; every face is offset 0.07 m from the voxel borders, so no lattice point of the map is merged with
another one by the map's voxel grids.  The map spans x in [-12, 12], the scan x in [-8, 8]; the scan is taken into the sensor
frame by the inverse of POSE and matched from a zero guess.

Why the faces are rough.  On ideal planes every normal has an exactly zero component along a free axis: AtA is exactly
singular there, cv::solve's QR reports it and the step is zero before the projection sees it.  A sensor never delivers that,
and neither do these scenes: every point is moved by up to ROUGH = 4 mm along its face's normal (edges: across the edge).
The fitted normals then tilt by some 1e-2, the free directions get small non-zero eigenvalues, and the unprojected solution X is
noise amplified along them: what matP exists to remove, and what makes a skipped projection visible (`proj_gap`).

Each scene states its preconditions (`expect`); tests assert them, with step_ref, on the recorded sums of the side under test."""
import numpy as np

import step_ref
from helpers import make_small_scene, small_params

POSE = np.array([0.004, -0.006, 0.01, 0.05, -0.04, 0.03])          # roll, pitch, yaw, x, y, z of the sensor in the map
OFF = 0.07                                                          # distance of a face from the voxel border
ROUGH = 0.004
LEAF_C, LEAF_S = 0.2, 0.4

# corridor_endwall(n): members of the family picked by a search on the oracle (lambda_min rises by ~0.9 per end-wall point)
N_JUST_BELOW = 112         # lambda_min  97.96 on the oracle
N_IN_ZONE = 116            # lambda_min 101.57, shortcut threshold 100 + 1e-4 * 28 243 = 102.82
N_CLEAR = 136              # lambda_min 115.07

BREAK_SETTINGS = {"break": {}, "nobreak": dict(icp_max_iters=6, icp_disable_break=1)}


def _rot_zyx(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, sy * sr + cy * sp * cr],
                     [sy * cp, cy * cr + sy * sp * sr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def _centres(lo, hi, leaf):
    """voxel centres of the cells of size leaf that lie inside [lo, hi]"""
    k = np.arange(int(np.ceil(lo / leaf - 1e-9)), int(np.floor(hi / leaf + 1e-9)))
    return (k + 0.5) * leaf


def _face(rng, axis, value, u_rng, v_rng, leaf=LEAF_S):
    """lattice on the plane coord[axis] = value; u, v are the two other axes in ascending order"""
    u, v = np.meshgrid(_centres(*u_rng, leaf), _centres(*v_rng, leaf), indexing="ij")
    n = u.size
    p = np.zeros((n, 3))
    ua, va = [a for a in range(3) if a != axis]
    p[:, ua] = u.ravel() + rng.uniform(-0.3, 0.3, n) * leaf
    p[:, va] = v.ravel() + rng.uniform(-0.3, 0.3, n) * leaf
    p[:, axis] = value + rng.uniform(-ROUGH, ROUGH, n)
    return p


def _edge_x(rng, y, z, x_rng):
    """lattice on the line parallel to x through (y, z)"""
    x = _centres(*x_rng, LEAF_C)
    n = x.size
    return np.stack([x + rng.uniform(-0.3, 0.3, n) * LEAF_C, y + rng.uniform(-ROUGH, ROUGH, n), z + rng.uniform(-ROUGH, ROUGH, n)], 1)


def _cloud(parts):
    xyz = np.concatenate(parts)
    out = np.zeros((len(xyz), 4), np.float32)
    out[:, :3] = xyz
    return out


def _to_sensor(xyz):
    R = _rot_zyx(*POSE[:3])
    return (np.asarray(xyz) - POSE[3:]) @ R                         # rows: R^T (p - t)


def _scene(name, map_corner, map_surf, corner, surf, expect):
    return dict(name=name, staged=False, map_corner=_cloud(map_corner), map_surf=_cloud(map_surf),
                corner=_cloud([_to_sensor(np.concatenate(corner))]), surf=_cloud([_to_sensor(np.concatenate(surf))]),
                guess=np.zeros(6, np.float32), expect=expect)


def _corridor_parts(rng, x_rng):
    surf = [_face(rng, 2, OFF, x_rng, (-1.6, 1.6)),                 # floor z = 0
            _face(rng, 1, 2.0 + OFF, x_rng, (0.4, 3.2)),            # walls y = +-2 (kept 0.4 m clear of the floor: no mixed neighbourhoods)
            _face(rng, 1, -2.0 - OFF, x_rng, (0.4, 3.2))]
    corner = [_edge_x(rng, sy * (2.0 + OFF), z + OFF, x_rng) for sy in (1, -1) for z in (0.0, 3.0)]
    return corner, surf


def _end_walls(rng):
    """end walls x = +-6, y in [-1.6, 1.6], z in [0.4, 4.0]: 2 x 72 lattice points, the two walls interleaved"""
    a = _face(rng, 0, 6.0 + OFF, (-1.6, 1.6), (0.4, 4.0))
    b = _face(rng, 0, -6.0 - OFF, (-1.6, 1.6), (0.4, 4.0))
    return np.stack([a, b], 1).reshape(-1, 3)


def corridor():
    """floor and two walls, four edges parallel to x: x is unconstrained"""
    rng = np.random.default_rng(20260)
    mc, ms = _corridor_parts(rng, (-12.0, 12.0))
    sc, ss = _corridor_parts(rng, (-8.0, 8.0))
    return _scene("corridor", mc, ms, sc, ss, dict(n_below=1, lam_min=(0.0, 50.0), degenerate=True))


def corridor_endwall(n, lam_min=None):
    """the corridor plus end walls at x = +-6 in the map; the first n end-wall lattice points are in the scan too"""
    rng = np.random.default_rng(20260)
    mc, ms = _corridor_parts(rng, (-12.0, 12.0))
    sc, ss = _corridor_parts(rng, (-8.0, 8.0))
    ms.append(_end_walls(rng))
    ss.append(_end_walls(rng)[:n])
    below = lam_min is None or lam_min[1] < step_ref.EIG_THRESHOLD
    return _scene(f"corridor_endwall({n})", mc, ms, sc, ss,
                  dict(n_below=1 if below else 0, lam_min=lam_min or (0.0, 99.5), degenerate=below))


def endwall_just_below():
    return corridor_endwall(N_JUST_BELOW, (97.0, 99.5))             # Jacobi runs, degenerate


def endwall_in_zone():
    return corridor_endwall(N_IN_ZONE, (100.5, 102.0))              # the LDL^T shortcut fails, Jacobi runs, NOT degenerate


def endwall_clear():
    return corridor_endwall(N_CLEAR, (110.0, np.inf))               # the shortcut holds


def slab():
    """floor and ceiling only: x, y and yaw are unconstrained.  The scan's corner points lie more than 1 m from every map
    corner: the feature-count gate passes, no corner row is selected.
    Seed: the first one from 20261 on at which the ORACLE's own step error is at least two float32 spacings of the pose in both
    classes (5.9 and 3.1).  Float32 solvers scatter by 1 - 16 spacings on this family (three directions removed, |X - PX| of
    some 1e-2 leaking through eigenvectors good to a few 2^-24); where the oracle happens to land below one spacing, the bar
    of tests/test_gpu_step.py (4 max(E_orc, U)) would measure that luck and not float32"""
    rng = np.random.default_rng(20262)
    ms = [_face(rng, 2, OFF, (-12.0, 12.0), (-2.0, 2.0)), _face(rng, 2, 3.0 + OFF, (-12.0, 12.0), (-2.0, 2.0))]
    ss = [_face(rng, 2, OFF, (-8.0, 8.0), (-2.0, 2.0)), _face(rng, 2, 3.0 + OFF, (-8.0, 8.0), (-2.0, 2.0))]
    mc = [_edge_x(rng, 2.0 + OFF, OFF, (8.0, 12.0))]
    sc = [_edge_x(rng, OFF, 1.4 + OFF, (-2.0, 2.0))]
    return _scene("slab", mc, ms, sc, ss, dict(n_below=3, lam_min=(0.0, 90.0), degenerate=True, outside=(90.0, 110.0)))


def boxes(pkg, oracle):
    """the well-conditioned case: helpers.make_small_scene through the staged path (raw scan -> features -> DS -> match)"""
    sc = make_small_scene(pkg, oracle)
    sc.update(name="boxes", staged=True, expect=dict(n_below=0, lam_min=(110.0, np.inf), degenerate=False))
    return sc


FEATURE_SCENES = dict(corridor=corridor, endwall_just_below=endwall_just_below, endwall_in_zone=endwall_in_zone,
                      endwall_clear=endwall_clear, slab=slab)
SCENE_NAMES = list(FEATURE_SCENES) + ["boxes"]
_cache = {}


def get(name, pkg, oracle):
    """the scene `name`, built once per process and never modified"""
    if name not in _cache:
        _cache[name] = boxes(pkg, oracle) if name == "boxes" else FEATURE_SCENES[name]()
    return _cache[name]


def load(h, sc):
    h.map_set(sc["map_corner"], sc["map_surf"])


def match(pkg, h, sc):
    """one scan match of the scene on handle h (its map already loaded): result dict + the recorded sums and pose trace"""
    A = pkg._abi
    if sc["staged"]:
        h.scan_upload(sc["scan"]); h.scan_organize(); h.scan_extract(); h.scan_downsample()
        r = h.scan_match(sc["guess"])
    else:
        r = h.scan_to_map(sc["corner"], sc["surf"], sc["guess"])
    r["jtj"] = h.debug_get(A.DBG_ICP_JTJ, np.float32).reshape(-1, 27)
    r["trace"] = h.debug_get(A.DBG_ICP_POSE_TRACE, np.float32).reshape(-1, 6)
    return r


def run(pkg, lib, sc, **params):
    h = pkg.LidarHotpath(lib, **small_params(**params))
    try:
        load(h, sc)
        return match(pkg, h, sc)
    finally:
        h.close()


def check_preconditions(sc, r):
    """hard assertions on the recorded sums of the side that produced r; returns step_ref's verdict on iteration 0"""
    e = sc["expect"]
    assert r["status"] == 0 and len(r["jtj"]) == r["iters"] >= 1 and len(r["trace"]) == r["iters"] + 1, (sc["name"], r["status"], r["iters"])
    assert r["n_sel"][0] >= 50, (sc["name"], r["n_sel"])
    s0 = step_ref.gn_step(r["jtj"][0], 0)
    w = s0.eigenvalues
    assert int((w < step_ref.EIG_THRESHOLD).sum()) == e["n_below"], (sc["name"], w)
    assert e["lam_min"][0] <= w[0] <= e["lam_min"][1], (sc["name"], w)
    assert np.abs(w - step_ref.EIG_THRESHOLD).min() >= 0.5, (sc["name"], w)          # the verdict is decidable in float32
    if "outside" in e:
        assert not ((w >= e["outside"][0]) & (w <= e["outside"][1])).any(), (sc["name"], w)
    assert s0.degenerate == e["degenerate"]
    if e["degenerate"]:
        assert s0.proj_gap >= 1e-3, (sc["name"], s0.proj_gap)
    return s0


def step_errors(r):
    """|(trace[i+1] - trace[i]) - step64(jtj[i])| per recorded iteration: (rotation part [iters,3], translation part [iters,3]),
    with step_ref's flags.  The trace is float32; the differences are taken in float64."""
    steps, degenerate, converged, iters = step_ref.replay(r["jtj"], break_enabled=False)
    t = r["trace"].astype(np.float64)
    e = np.abs((t[1:] - t[:-1]) - np.stack([s.step for s in steps]))
    return e[:, :3], e[:, 3:], steps, degenerate
