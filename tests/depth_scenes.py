"""TEST INFRASTRUCTURE — hand-built scenes for the LiDAR depth association (tests/test_depth_scenes.py checks the scenes
themselves on the CPU, tests/test_gpu_depth_edges.py runs them on the device).

Every scene is a body-frame cloud for DepthRegister.set_cloud plus the features of one get_depth call.  Points are placed
at the centre of a range-image bin (row = elevation, column = atan2(x, y), 0.5 degrees each) unless a scene says
otherwise, so none of them lies near a rounding boundary of the range image.  Body axes: x forward, y left, z up; a
feature (u, v, 1) looks along (1, -u, -v).  Never imported by the product package."""
import math

import numpy as np

import depth_ref as R

F32 = np.float32
IDENT = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
POSE2 = (1.0, -0.5, 0.2, 0.05, -0.03, 0.4)
CLASSES = ("inside", "clamp_high", "clamp_low", "spread", "small_s", "near", "far", "collinear", "duplicate", "mirrored")


def bin_dir(row, col):
    """unit direction (float64) of the centre of bin (row, col)"""
    el, ca = math.radians(row * 0.5 - 90.0), math.radians(col * 0.5)
    return np.array([math.cos(el) * math.sin(ca), math.cos(el) * math.cos(ca), math.sin(el)])


def bin_point(row, col, rng, intensity=1.0):
    d = bin_dir(row, col) * rng
    return [d[0], d[1], d[2], intensity]


def ray_bin(f):
    """the bin a feature's ray falls in"""
    v = R.feature_rays([f])[0].astype(np.float64)
    row = (math.degrees(math.atan2(v[2], math.hypot(v[0], v[1]))) + 90.0) / 0.5
    col = math.degrees(math.atan2(v[0], v[1])) / 0.5
    return int(round(row)), int(round(col))


def _cloud(pts):
    return np.array(pts, np.float64).reshape(-1, 4).astype(np.float32)


# ------------------------------------------------------------------------------------------------------- branches
# offsets (rows, columns, range added to the feature's base range) of a class's cluster around the ray's bin
_AROUND = ((2, 0), (-1, 2), (-1, -2))                            # a triangle around the ray, about 1 degree away
_ONE_SIDE = ((1, -2), (1, 2), (3, 0))                            # all three above the ray, the last one outermost
_CLUSTER = {
    "inside": [(dr, dc, a) for (dr, dc), a in zip(_AROUND, (0.0, 0.3, -0.2))],
    "clamp_high": [(dr, dc, a) for (dr, dc), a in zip(_ONE_SIDE, (0.0, 0.0, -0.5))],     # the plane rises towards the ray
    "clamp_low": [(dr, dc, a) for (dr, dc), a in zip(_ONE_SIDE, (0.0, 0.0, 0.5))],
    "spread": [(dr, dc, a) for (dr, dc), a in zip(_AROUND, (0.0, 2.5, 0.0))],
    "small_s": [(dr, dc, a) for (dr, dc), a in zip(_AROUND, (0.0, 0.01, -0.01))],         # base range 0.4
    "near": [(dr, dc, a) for (dr, dc), a in zip(_AROUND, (0.0, 0.02, -0.02))],            # base range 2.9
    "duplicate": [(dr, dc, a) for (dr, dc), a in zip(_AROUND, (0.0, 0.3, -0.2))],         # + the first point once more
    "mirrored": [(2, 2, 0.0), (-2, -2, 0.1), (2, -2, 0.25), (-2, 2, 0.4)],
}
_FAR_DIRS = ((6, 0), (-6, 0), (0, 7), (0, -7))                    # candidates for the far third point, about 3 degrees away


def branch_features():
    u, v = np.meshgrid(np.linspace(-0.9, 0.9, 15), np.linspace(-0.6, 0.6, 10))
    return np.stack([u.ravel(), v.ravel(), np.ones(150)], 1).astype(np.float32)


def branches():
    """-> (body-frame cloud [480, 4], features [150, 3], class name per feature, cloud indices of each feature's cluster)"""
    feats = branch_features()
    V = R.feature_rays(feats).astype(np.float64)
    labels = [CLASSES[k % 10] for k in range(150)]
    pts, own = [], []
    for k, f in enumerate(feats):
        r0, c0 = ray_bin(f)
        cls = labels[k]
        base = {"small_s": 0.4, "near": 2.9}.get(cls, 8.0 + 0.25 * (k % 17))
        first = len(pts)
        if cls == "far":
            # two points close to the ray, the third beyond the acceptance arc on the side farthest from the other rays
            others = np.delete(V, k, 0)
            dr, dc = max(_FAR_DIRS, key=lambda o: np.degrees(np.arccos(np.clip(others @ bin_dir(r0 + o[0], c0 + o[1]), -1, 1))).min())
            cluster = [(1, 1, 0.0), (-1, -1, 0.2), (dr, dc, 0.1)]
        elif cls == "collinear":
            # three points of one column (one vertical plane) on a straight line across the line of sight of its middle one
            cluster = [(dr, 2, base / math.cos(math.radians(0.5 * dr)) - base) for dr in (-2, 0, 2)]
        else:
            cluster = _CLUSTER[cls]
        for dr, dc, add in cluster:
            pts.append(bin_point(r0 + dr, c0 + dc, base + add, float(k)))
        if cls == "duplicate":
            pts.append(list(pts[first]))
        own.append(list(range(first, len(pts))))
    return _cloud(pts), feats, labels, own


def branch_taken(sphere, nbr, sqd, V, depth):
    """which branch of steps 6-7 one feature takes, from a search result and the published depth"""
    if (nbr < 0).any():
        return "none"
    if not sqd[2] < R.DIST_SQ_THRESHOLD:
        return "far"
    P = sphere[nbr].astype(np.float32)
    r = P[:, 3]
    A, B, Cc = (P[i, :3] * r[i] for i in range(3))
    N = np.cross((A - B).astype(np.float32), (B - Cc).astype(np.float32)).astype(np.float32)
    with np.errstate(all="ignore"):
        s = F32((N[0] * A[0] + N[1] * A[1]) + N[2] * A[2]) / F32((N[0] * V[0] + N[1] * V[1]) + N[2] * V[2])
    if F32(r.max() - r.min()) > 2:
        return "spread"
    if s <= 0.5:
        return "small_s"
    if not np.isfinite(s) and not s > 0:
        return "nan"
    clamp = "clamp_high" if F32(s - r.max()) > 0 else "clamp_low" if F32(s - r.min()) < 0 else "inside"
    return clamp if depth > 3.0 else "near"


def collinearity(sphere, nbr):
    """|N| / (|A - B| |B - C|) of three neighbours in float64: 0 for collinear points"""
    P = sphere[nbr].astype(np.float64)
    A, B, Cc = (P[i, :3] * P[i, 3] for i in range(3))
    return np.linalg.norm(np.cross(A - B, B - Cc)) / (np.linalg.norm(A - B) * np.linalg.norm(B - Cc))


def class_counts(labels, own, sphere_idx, sphere, nbr, sqd, V, depth):
    """per class of `branches`, how many of its features behave as built: neighbours inside their own cluster and the
    intended branch taken (collinear: the three collinear points accepted, on whichever branch the rounding noise of their
    normal leads to; duplicate: the lower of the two equal cloud indices kept, plane intersection inside; mirrored: three
    of the four accepted with a depth)"""
    counts = {c: 0 for c in CLASSES}
    taken = []
    for k, cls in enumerate(labels):
        b = branch_taken(sphere, nbr[k], sqd[k], V[k], depth[k])
        taken.append(b)
        if (nbr[k] < 0).any() or not set(sphere_idx[nbr[k]]) <= set(own[k]):
            continue
        if cls == "collinear":
            ok = b not in ("none", "far", "spread") and collinearity(sphere, nbr[k]) < 1e-4
        elif cls == "duplicate":
            ok = b == "inside" and own[k][0] in sphere_idx[nbr[k]] and own[k][-1] not in sphere_idx[nbr[k]]
        elif cls == "mirrored":
            ok = b in ("inside", "clamp_high", "clamp_low")
        else:
            ok = b == cls
        counts[cls] += bool(ok)
    return counts, taken


# ------------------------------------------------------------------------------------------------------------ ties
AXIS_FEATURE = np.array([[0.0, 0.0, 1.0]], np.float32)            # looks along body x: bin (180, 180)


def _mirrored(row, dcol, rng):
    p = np.array(bin_point(row, 180 - dcol, rng), np.float64).astype(np.float32)     # y > 0: the lower column
    q = p.copy(); q[1] = -q[1]
    return [p, q]


def ties():
    """identity pose, the feature on the optical axis.  Pairs (x, +-y, z) are bit-equally far from it; the +y one has the
    lower column, hence the lower sphere index.  -> {name: cloud}
    pairs:            the two nearest tie, and the third place is a tie as well
    single_then_pair: one nearest point, then a tie for places two and three, then a tie for the place that is dropped
    repeated:         `pairs` with its cloud point 2 once more in front (indices 0 and 3, one bin, equal distance)"""
    far = [p for row, dcol, rng in ((176, 6, 9.0), (185, 7, 11.0), (174, 3, 9.5), (187, 8, 10.5)) for p in _mirrored(row, dcol, rng)]
    pairs = _mirrored(181, 2, 10.0) + _mirrored(178, 3, 10.4) + _mirrored(183, 4, 9.7) + far
    on_axis = np.array(bin_point(181, 180, 10.2), np.float64).astype(np.float32)
    on_axis[1] = 0.0                                               # cos(90 deg) in floating point is not 0
    single = [on_axis] + _mirrored(179, 2, 10.0) + _mirrored(182, 3, 9.6) + far
    out = {"pairs": np.array(pairs, np.float32), "single_then_pair": np.array(single, np.float32)}
    out["repeated"] = np.concatenate([out["pairs"][2:3], out["pairs"]])
    return out


# ----------------------------------------------------------------------------------------------------------- small
def _ring(n, rng=10.0, row=182):
    """n points in n bins around the optical axis"""
    return [bin_point(row + (k % 3) * 2 - 2, 180 + 3 * (k - n // 2), rng + 0.1 * k) for k in range(n)]


SMALL_FEATURES = np.array([[0.0, 0.0, 1.0], [0.02, -0.01, 1.0], [-0.05, 0.03, 1.0]], np.float32)


def small():
    """identity pose.  -> {name: cloud}; what each must give is in SMALL_EXPECT"""
    ten = np.nextafter(F32(10.0), F32(np.inf))
    return {
        "nine_bins": _cloud(_ring(9)),
        "ten_bins": _cloud(_ring(10)),
        "one_point": _cloud(_ring(1)),
        "all_behind": _cloud([[-p[0], p[1], p[2], p[3]] for p in _ring(12)]),
        "origin_plus_10": _cloud([[0.0, 0.0, 0.0, 1.0]] + _ring(10)),
        "origin_plus_9": _cloud(_ring(9) + [[0.0, 0.0, 0.0, 1.0]]),            # 10 sphere entries, 9 of them points
        "x_zero": _cloud(_ring(10) + [[0.0, 0.0, 2.0, 1.0], [0.0, 3.0, 0.0, 1.0], [0.0, -3.0, 0.5, 1.0]]),
        # |y / x| and |z / x| exactly 10 are kept, the next float above 10 is cut (x = 1 and x = 0.5: the ratios are exact)
        "ratio_ten": np.concatenate([_cloud(_ring(10)), np.array([[1.0, 10.0, 0.0, 1.0], [0.5, -5.0, 0.0, 1.0], [1.0, 0.0, 10.0, 1.0], [0.5, 0.0, -5.0, 1.0],
                                                                  [1.0, ten, 0.25, 1.0], [1.0, -ten, 0.25, 1.0], [1.0, 0.25, ten, 1.0], [1.0, 0.25, -ten, 1.0]], np.float32)]),
    }


# occupied bins, and whether get_depth searches (10 or more sphere entries)
SMALL_EXPECT = {"nine_bins": (9, False), "ten_bins": (10, True), "one_point": (1, False), "all_behind": (0, False), "origin_plus_10": (11, True),
                "origin_plus_9": (10, True), "x_zero": (10, True), "ratio_ten": (14, True)}


# -------------------------------------------------------------------------------------------------------- features
def features():
    """identity pose.  A cluster around the optical axis and points at the highest and lowest elevations the field of view
    keeps (rows 12-13 and 347-348), 60 m away so that a depth survives the d > 3 test.  -> (cloud, features):
    the zero vector, (0, +-20, 1) and (0, +-15.3, 1) whose search bands are clipped at rows 0 and 359 (the latter pair
    within the acceptance arc of the polar points), the axis, a feature looking backwards"""
    pts = _ring(12)
    for row in (347, 348, 13, 12):
        pts += [bin_point(row, col, 60.0 + 0.01 * col) for col in (166, 173, 180, 187, 194)]
    f = np.array([[0, 0, 0], [0, 20, 1], [0, -20, 1], [0, 15.3, 1], [0, -15.3, 1], [0, 0, 1], [0, 0, -1]], np.float32)
    return _cloud(pts), f


def band_rows(f, half=7):
    """the rows get_depth's band search reads for one feature, before clipping"""
    v = R.feature_rays([f])[0].astype(np.float64)
    fr = (math.degrees(math.atan2(v[2], math.hypot(v[0], v[1]))) + 90.0) / 0.5
    return math.floor(fr - half), math.ceil(fr + half)


# ---------------------------------------------------------------------------------------------------------- checks
def boundary_margin(local):
    """smallest distance, in bins, of the row / column value of any point the range image takes from a rounding
    boundary (k + 0.5)"""
    with np.errstate(all="ignore"):
        skip = (local[:, 0] < 0) | (np.abs(local[:, 1] / local[:, 0]) > 10) | (np.abs(local[:, 2] / local[:, 0]) > 10)
    local = local[~skip]
    if len(local) == 0:
        return 0.5
    x, y, z = (local[:, k].astype(np.float64) for k in range(3))
    rr = (np.degrees(np.arctan2(z, np.sqrt(x * x + y * y))) + 90.0) / 0.5
    cc = np.degrees(np.arctan2(x, y)) / 0.5
    return float(min(np.abs(rr - np.floor(rr) - 0.5).min(), np.abs(cc - np.floor(cc) - 0.5).min()))


# ---------------------------------------------------------------------------------------------------------- window
def lattice_cloud(n, seed):
    """n points, one per 0.2 m voxel: a 0.5 m lattice in front of the sensor with 0.05 m jitter, every second point
    mirrored to x < 0 so that the field-of-view cut drops half"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    g = np.stack([4.1 + 0.5 * (k // 400), -4.9 + 0.5 * (k % 20), -4.9 + 0.5 * ((k // 20) % 20)], 1)
    p = g + rng.uniform(-0.05, 0.05, (n, 3))
    p[1::2, 0] = -p[1::2, 0]
    return np.concatenate([p, rng.uniform(0, 100, (n, 1))], 1).astype(np.float32)


def window_sequence():
    """the clouds of the window test in order: sizes 0, 1, 1023, 1024, 1025, 2049, 0, 3000 (all behind), 7"""
    seq = [lattice_cloud(n, 900 + i) for i, n in enumerate((0, 1, 1023, 1024, 1025, 2049, 0))]
    behind = lattice_cloud(3000, 950)
    behind[:, 0] = -np.abs(behind[:, 0])
    return seq + [behind, lattice_cloud(7, 960)]


WINDOW_KEPT = (0, 1, 512, 512, 513, 1025, 0, 0, 4)           # points of each cloud that survive the field-of-view cut


def window_pose(k):
    return (0.05 * k, 0.02 * k, 0.0, 0.0, 0.01 * k, 0.02 * k)


def window_stamp(k):
    """0.4 s apart: with window_s = 1.0 the window holds three clouds and pops one at every callback from the fourth on"""
    return 10.0 + 0.4 * k
