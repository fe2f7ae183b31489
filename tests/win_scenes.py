"""Scenes of the sliding-window solve's tests (tests/win_ref.py).  A scene is a script over anything with
set_block / add_projection / add_imu / set_prior: a window whose poses follow from seeded IMU samples through the numpy
preintegration, features seen from it with pixel noise, an optional synthetic full-rank prior, and the state perturbed
away from the truth so that the solve has work to do.  Ids are tests/marg_ref.py's."""
import numpy as np

import marg_ref as M
import win_ref as R
from marg_ref import ID_EX, ID_FEATURE, ID_POSE, ID_SPEEDBIAS, ID_TD

ID_PAD = 48                      # free blocks no factor names
G = np.array([0.0, 0.0, 9.8])
FRAME_SAMPLES, SAMPLE_DT = 6, 0.02       # five integration steps of 20 ms per frame interval


def _extrinsic(rs):
    ric = np.array([[0., 0., 1.], [-1., 0., 0.], [0., -1., 0.]])
    qw = np.sqrt(1 + ric[0, 0] + ric[1, 1] + ric[2, 2]) / 2
    q = np.array([(ric[2, 1] - ric[1, 2]) / (4 * qw), (ric[0, 2] - ric[2, 0]) / (4 * qw), (ric[1, 0] - ric[0, 1]) / (4 * qw), qw])
    ex = np.r_[0.05, -0.02, 0.03, M.quat_mul(q, M.rand_quat(rs, 0.02))]
    ex[3:] /= np.linalg.norm(ex[3:])
    return ex


def make_scene(seed, frames, frames_seen, use_td=True, free_ex=True, imu=True, prior=True, constant_features=(), first_frames=(0,), pad=(), skip_imu=(),
               perturb=1.0, count=None, zero_depth=None, params=None):
    """-> dict(params, ops): ops are ("block", id, values, flags), ("proj", record), ("imu", record), ("prior", dict)"""
    rs = np.random.RandomState(seed)
    ba, bg = rs.normal(0, 0.02, 3), rs.normal(0, 0.002, 3)
    pose, sb, pre = np.zeros((frames, 7)), np.zeros((frames, 9)), []
    pose[0] = np.r_[rs.normal(0, 0.02, 3), M.rand_quat(rs, 0.05)]
    sb[0] = np.r_[3.0, rs.normal(0, 0.05, 2), ba, bg]
    for k in range(frames - 1):
        Rk = M.rot(pose[k, 3:])
        a0, w0 = Rk.T @ G + rs.normal(0, 0.5, 3), rs.normal(0, 0.1, 3)
        accs = [a0 + rs.normal(0, 0.05, 3) + ba for _ in range(FRAME_SAMPLES)]
        gyrs = [w0 + rs.normal(0, 0.01, 3) + bg for _ in range(FRAME_SAMPLES)]
        p = R.preintegrate([SAMPLE_DT] * FRAME_SAMPLES, accs, gyrs, ba, bg)
        dt = p["sum_dt"]
        pose[k + 1, :3] = pose[k, :3] + sb[k, :3] * dt - 0.5 * G * dt * dt + Rk @ p["delta_p"]
        pose[k + 1, 3:] = M.quat_mul(pose[k, 3:], p["delta_q"])
        pose[k + 1, 3:] /= np.linalg.norm(pose[k + 1, 3:])
        sb[k + 1] = np.r_[sb[k, :3] - G * dt + Rk @ p["delta_v"], ba + rs.normal(0, 1e-4, 3), bg + rs.normal(0, 1e-5, 3)]
        pre.append(p)
    ex, td = _extrinsic(rs), 0.01
    Rc, feats = M.rot(ex[3:]), []
    for f in range(len(frames_seen)):
        start = first_frames[f % len(first_frames)]
        depth = rs.uniform(4, 12)
        pc = np.r_[rs.uniform(-0.4, 0.4), rs.uniform(-0.3, 0.3), 1.0] * depth
        pw = M.rot(pose[start, 3:]) @ (Rc @ pc + ex[:3]) + pose[start, :3]
        obs = []
        for j in range(start, min(start + frames_seen[f], frames)):
            pj = Rc.T @ (M.rot(pose[j, 3:]).T @ (pw - pose[j, :3]) - ex[:3])
            uv = pj[:2] / pj[2] + rs.normal(0, 0.5 / M.FOCAL_LENGTH, 2)
            obs.append(dict(frame=j, point=np.r_[uv, 1.0], velocity=rs.normal(0, 0.3, 2), cur_td=td + rs.normal(0, 1e-3), uv_y=float(240 + M.FOCAL_LENGTH * uv[1])))
        feats.append(dict(start=start, inv_dep=float(1.0 / depth * (1 + perturb * rs.normal(0, 0.02))), obs=obs))
    # the state the solve starts from: the truth perturbed
    s = 1e-2 * perturb
    pose0, sb0, ex0 = pose.copy(), sb.copy(), ex.copy()
    for k in range(frames):
        pose0[k, :3] += rs.normal(0, s, 3)
        pose0[k, 3:] = M.quat_mul(pose[k, 3:], M.rand_quat(rs, s))
        sb0[k] += np.r_[rs.normal(0, s, 3), rs.normal(0, 0.1 * s, 3), rs.normal(0, 0.01 * s, 3)]
    ex0[:3] += rs.normal(0, 0.1 * s, 3)
    ex0[3:] = M.quat_mul(ex[3:], M.rand_quat(rs, 0.1 * s))
    ops = []
    for k in range(frames):
        ops += [("block", ID_POSE + k, pose0[k], 0), ("block", ID_SPEEDBIAS + k, sb0[k], 0)]
    ops.append(("block", ID_EX, ex0, 0 if free_ex else R.CONSTANT))
    if use_td:
        ops.append(("block", ID_TD, [td + 1e-3 * perturb], 0))
    for k, size in enumerate(pad):
        ops.append(("block", ID_PAD + k, rs.normal(0, 1, size), 0))
    recs = []
    for k, f in enumerate(feats):
        for o in f["obs"][1:]:
            recs.append(M._rec(ID_POSE + f["start"], ID_POSE + o["frame"], ID_FEATURE + k, f["obs"][0], o, ID_TD if use_td else -1))
    recs = recs[:count] if count else recs
    for k, f in enumerate(feats):
        if any(r["feature"] == ID_FEATURE + k for r in recs):
            ops.append(("block", ID_FEATURE + k, [0.0 if zero_depth == k else f["inv_dep"]], R.CONSTANT if k in constant_features else R.ELIMINATED))
    if prior:
        ids = [ID_POSE, ID_SPEEDBIAS, ID_EX] + ([ID_TD] if use_td else [])
        x0 = [pose[0] + np.r_[rs.normal(0, 5e-3, 3), np.zeros(4)], sb[0] + rs.normal(0, 1e-3, 9), ex.copy()] + ([np.array([td])] if use_td else [])
        sizes = [len(v) for v in x0]
        scale = np.concatenate([[100.] * 6, [10.] * 3, [100.] * 3, [1000.] * 3, [100.] * 6] + ([[10.]] if use_td else []))
        n = len(scale)
        col = list(np.cumsum([0] + [M.local_size(z) for z in sizes])[:-1])
        ops.append(("prior", dict(J=np.diag(scale) + 0.1 * scale[None, :] * np.triu(rs.normal(0, 1, (n, n)), 1), r=rs.normal(0, 0.3, n), ids=ids, sizes=sizes, col=col,
                                  x0=x0)))
    if imu:
        for k, p in enumerate(pre):
            if k not in skip_imu:                            # estimator.cpp:740: a factor with sum_dt > 10 is left out by the caller
                ops.append(("imu", dict(pose_i=ID_POSE + k, speed_bias_i=ID_SPEEDBIAS + k, pose_j=ID_POSE + k + 1, speed_bias_j=ID_SPEEDBIAS + k + 1, **p)))
    ops += [("proj", r) for r in recs]
    P = dict(G=tuple(G))
    P.update(params or {})
    return dict(params=P, ops=ops)


def play(scene, target):
    for op in scene["ops"]:
        if op[0] == "block":
            target.set_block(op[1], op[2], op[3])
        elif op[0] == "proj":
            target.add_projection(op[1])
        elif op[0] == "imu":
            target.add_imu(op[1])
        else:
            target.set_prior(op[1])
    return target


def scene(name):
    if name == "two_frames":                     # 6 features, one IMU factor, the prior: D = 37
        return make_scene(1, 2, [2] * 6)
    if name == "three_td":                       # td and a free extrinsic: D = 52
        return make_scene(2, 3, [3, 2, 3, 3, 2, 3, 3, 3])
    if name == "three_plain":                    # no td, constant extrinsic: D = 45
        return make_scene(3, 3, [3, 2, 3, 3, 2, 3, 3, 3], use_td=False, free_ex=False)
    if name == "all_constant":                   # every feature has a lidar depth: nothing is eliminated
        return make_scene(4, 3, [3] * 6, constant_features=range(6))
    if name == "half_constant":
        return make_scene(5, 3, [3] * 6, constant_features=(0, 2, 4))
    if name == "eleven_frames":                  # a feature seen in all 11 frames, one with a single factor: D = 172
        return make_scene(6, 11, [11, 2, 5, 4, 7, 3], first_frames=(0, 9, 2, 5, 1, 3))
    if name == "skipped_imu":                    # the second interval's factor is left out
        return make_scene(7, 3, [3] * 6, skip_imu=(1,))
    if name == "no_prior":                       # gauge free
        return make_scene(8, 3, [3] * 8, prior=False, imu=False)
    if name in ("share", "share_plus_1", "two_shares_plus_1"):
        n = {"share": R.SHARE, "share_plus_1": R.SHARE + 1, "two_shares_plus_1": 2 * R.SHARE + 1}[name]
        return make_scene(9, 3, [3] * ((n + 1) // 2), count=n)
    if name == "chol_32":                        # D = 30 + 1 + 1 at the Cholesky's panel width (constant extrinsic)
        return make_scene(10, 2, [2] * 6, free_ex=False, pad=(1,))
    if name == "chol_33":
        return make_scene(11, 2, [2] * 6, free_ex=False, pad=(2,))
    if name == "chol_65":                        # 60 + 1 + 4: two panels and one column
        return make_scene(12, 4, [4, 3, 4, 2, 4, 3, 4, 4], free_ex=False, pad=(3, 1))
    if name == "chol_64":
        return make_scene(13, 4, [4, 3, 4, 2, 4, 3, 4, 4], free_ex=False, pad=(3,))
    if name == "zero_depth":                     # inv_dep == 0
        return make_scene(14, 2, [2] * 4, zero_depth=1)
    raise KeyError(name)


def shared_front_scene():
    """-> (blocks [(id, values)] in the order they are declared, projection records): the factor set the marginaliser and the
    window solve build one matrix from.  Three poses, the extrinsic, td and SHARE + 1 features with one
    projection factor with td each, from pose 0 to pose 1 or 2 in turn: 129 factors, one chunk boundary, D = 154."""
    win, feats = M.make_window(15, R.SHARE + 1, frames_seen=[3])
    blocks = [(ID_POSE + k, win["pose"][k]) for k in range(3)] + [(ID_EX, win["ex"]), (ID_TD, [win["td"]])]
    recs = []
    for k, f in enumerate(feats):
        blocks.append((ID_FEATURE + k, [f["inv_dep"]]))
        j = 1 + k % 2
        recs.append(M._rec(ID_POSE, ID_POSE + j, ID_FEATURE + k, f["obs"][0], f["obs"][j]))
    return blocks, recs


def shared_front_permutation(blocks, recs):
    """perm[c]: the marginaliser's column of the window solve's column c, when every pose_i and feature is dropped and the
    window solve has every block free.  The marginaliser orders the dropped blocks by first appearance in a drop set, then
    the kept blocks by first appearance (include/lvi_marg.h); the window solve keeps the order of declaration
    (include/lvi_win.h)."""
    size = {b: M.local_size(len(v)) for b, v in blocks}
    seen, dropped = [], []
    for r in recs:
        for key in ("pose_i", "pose_j", "ex", "feature", "td"):
            if r[key] not in seen:
                seen.append(r[key])
            if key in ("pose_i", "feature") and r[key] not in dropped:
                dropped.append(r[key])
    col, pos = {}, 0
    for b in dropped + [b for b in seen if b not in dropped]:
        col[b] = pos
        pos += size[b]
    return np.array([col[b] + k for b, _ in blocks for k in range(size[b])])


SYSTEM_SCENES = ["two_frames", "three_td", "three_plain", "all_constant", "half_constant", "eleven_frames", "skipped_imu", "no_prior", "share", "share_plus_1",
                 "two_shares_plus_1", "chol_32", "chol_33", "chol_64", "chol_65"]
F64_ONLY = ("eleven_frames", "share", "share_plus_1", "two_shares_plus_1", "chol_64", "chol_65")     # too slow in mpmath: compared with float64 at the floor alone
SOLVE_SCENES = ["two_frames", "three_td", "three_plain", "half_constant"]                            # candidates for a decision-sequence comparison
STEP_RADII = (1e6, 1e4, 1.0)                     # the three step kinds on `two_frames`: Gauss-Newton inside, the interpolated leg, the Cauchy step cut

RETRY_PARAMS = dict(min_diagonal=1e-30, initial_mu=1e-300, min_mu=1e-300)           # tests/test_win_ref.py says why these force seven retries

_cache = {}


def problem(name, X, **params):
    sc = scene(name)
    P = dict(sc["params"])
    P.update(params)
    return play(sc, R.Problem(X, **P))


def system_reference(name):
    """-> (float64 system, mpmath system or None) at the declared values"""
    key = ("sys", name)
    if key not in _cache:
        pf = problem(name, R.F64)
        pm = None if name in F64_ONLY else problem(name, R.MP)
        _cache[key] = (pf.system(pf.x0()), pm.system(pm.x0()) if pm else None)
    return _cache[key]


def solve_reference(name, **params):
    """-> (float64 solve, mpmath solve), computed once per (scene, parameters)"""
    key = ("solve", name, tuple(sorted(params.items())))
    if key not in _cache:
        _cache[key] = tuple(R.solve(problem(name, X, **params)) for X in (R.F64, R.MP))
    return _cache[key]


def solve_reference_f64(name, **params):
    """-> (float64 solve, None): for runs too long for mpmath"""
    key = ("solve64", name, tuple(sorted(params.items())))
    if key not in _cache:
        _cache[key] = (R.solve(problem(name, R.F64, **params)), None)
    return _cache[key]


def admitted():
    """the scenes of SOLVE_SCENES whose float64 and mpmath runs take the same decisions with every margin at least 1000 x the
    distance between the two arithmetics (tests/test_win_ref.py asserts that this is what the list holds)"""
    if "admitted" not in _cache:
        out = []
        for name in SOLVE_SCENES:
            f, m = solve_reference(name)
            if R.decisions(f) == R.decisions(m) and R.min_margin(f, m)[0] >= 1000.0:
                out.append(name)
        _cache["admitted"] = out
    return _cache["admitted"]
