"""TEST INFRASTRUCTURE — the keyframe scenes of the loop-closure tests (tests/test_loop_cpu.py, tests/test_gpu_loop.py).

Two passes over the same stretch of synth.loop_pose, made by the oracle as in test_gpu_gmap.py: N1 keys of a first pass
(stamps 0, 1, …) and N2 keys of a second pass more than 30 s later (stamps 100, 101, …) whose poses carry a known drift.
SEARCH (historyKeyframeSearchNum) is reduced to 3 so that the float64 reference stays affordable.

    revisit_a / revisit_b   the drifted revisit, two drifts (a few decimetres, about 1 degree): accept
    turned                  the revisit's pose turned by 90 degrees and moved by 25 m: the clouds do not overlap as placed
                            and ICP ends far from any fit: reject
    other_place             a cloud of another shape (the keyframe stretched by 1.6 x 0.6): no rigid motion fits: reject

Never imported by the product package."""
import numpy as np

import gmap_ref as G
import loop_ref as LR
from helpers import small_params

N1, N2 = 12, 3
SEARCH = 3
LEAF = 0.4
MAX_CORR = 30.0
FITNESS_GATE = 0.3
PRE = 6                                   # the first-pass key the second pass's middle key revisits
CUR = N1 + 1
DRIFTS = dict(revisit_a=(0.3, -0.2, 0.05, 0.004, -0.003, np.deg2rad(1.0)), revisit_b=(-0.25, 0.35, -0.04, -0.005, 0.002, np.deg2rad(-1.2)),
              turned=(20.0, 15.0, 0.0, 0.0, 0.0, np.deg2rad(90.0)), other_place=(0.0, 0.0, 0.0, 0.0, 0.0, 0.0))
ACCEPT = dict(revisit_a=True, revisit_b=True, turned=False, other_place=False)


def _keyframes(pkg, oracle, alphas, seeds, n_raw=16001):
    S = pkg.synth
    o = pkg.LidarHotpath(oracle, **small_params())
    out = []
    for a, sd in zip(alphas, seeds):
        pose = S.loop_pose(a, 0.01 * np.sin(sd), -0.01 * np.cos(sd)).astype(np.float32)
        o.scan_upload(S.make_scan(n_raw, pose, sd)); o.scan_organize(); o.scan_extract(); o.scan_downsample()
        c, s = o.get_scan_ds()
        out.append((c.copy(), s.copy(), pose))
    o.close()
    return out


def drift_matrix(name):
    return LR.rpy_matrix(*DRIFTS[name])


def drifted(pose, D):
    """the pose (roll, pitch, yaw, x, y, z) of D * T(pose)"""
    r, p, y, x, yy, z = [float(v) for v in pose]
    x, yy, z, r, p, y = LR.euler_of(D @ LR.rpy_matrix(x, yy, z, r, p, y))
    return np.array([r, p, y, x, yy, z], np.float32)


def base_passes(pkg, oracle):
    first = _keyframes(pkg, oracle, [0.2 + 0.15 * k for k in range(N1)], [900 + k for k in range(N1)])
    second = _keyframes(pkg, oracle, [0.2 + 0.15 * (5 + j) + 0.05 for j in range(N2)], [1900 + j for j in range(N2)])
    return first, second


def scene(name, passes):
    """-> dict(kfs = [(corner, surf, pose)] of N1 + N2 keys, stamps, D (the injected drift, None for other_place))"""
    first, second = passes
    D = drift_matrix(name)
    kfs = list(first)
    for c, s, p in second:
        if name == "other_place":
            c, s = c.copy(), s.copy()
            for a in (c, s):
                a["x"] *= np.float32(1.6); a["y"] *= np.float32(0.6)
        kfs.append((c, s, drifted(p, D)))
    stamps = [float(k) for k in range(N1)] + [100.0 + j for j in range(N2)]
    return dict(name=name, kfs=kfs, stamps=stamps, D=None if name == "other_place" else D)


def target_keys(pre, n_keys, search=SEARCH):
    return list(range(max(pre - search, 0), min(pre + search, n_keys - 1) + 1))


def submaps_ref(pkg, ora, kfs, cur, pre, leaf=LEAF, search=SEARCH):
    """the two submaps of loopFindNearKeyframes through gmap_ref: dicts of G.voxel plus 'fused'"""
    corners, surfs, poses = [k[0] for k in kfs], [k[1] for k in kfs], [k[2] for k in kfs]
    out = []
    for keys in ([cur], target_keys(pre, len(kfs), search)):
        f = G.fuse(ora, corners, surfs, poses, keys, G.CORNER_SURF)
        v = G.voxel(pkg, ora, f, leaf) if leaf > 0 else dict(overflow=True, pts=G.xyzi(f).copy())
        v["fused"] = f
        out.append(v)
    return out


def reference_pair(oracle, src, tgt, **kw):
    """the restatement in both precisions on [n, >= 3] clouds: (f32 result, float64 result)"""
    a = LR.icp(src[:, :3], tgt[:, :3], LR.nn_kdtree(oracle), max_corr_dist=MAX_CORR, precision="f32", **kw)
    b = LR.icp(src[:, :3], tgt[:, :3], LR.nn_reranked(oracle), max_corr_dist=MAX_CORR, precision="f64", **kw)
    return a, b


def gaps(Ta, fa, Tb, fb):
    """(rotation angle of the difference, norm of the translation difference, relative fitness difference) of a from b"""
    Ta, Tb = np.asarray(Ta, np.float64), np.asarray(Tb, np.float64)
    return LR.rot_angle(Ta, Tb), float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3])), abs(fa - fb) / abs(fb)
