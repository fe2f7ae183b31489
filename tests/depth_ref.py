"""TEST INFRASTRUCTURE — numpy f32 restatement of the feature tracker's LiDAR depth association:
lidar_callback (feature_tracker_node.cpp:273-377) and DepthRegister::get_depth (feature_tracker.h:116-331).

The PCL parts come from the CPU oracle: VoxelGrid = lvi_voxel_downsample, transformPointCloud = lvi_transform_cloud,
getTransformation = lvo_test_get_transformation, KdTreeFLANN 3-NN = the first 3 of lvo_test_kdtree_knn's 5.
atan2f is modelled as the correctly rounded value (float64 atan2 rounded to f32), as glibc's atan2f; roundf as half
away from zero.  pose6 = (x, y, z, roll, pitch, yaw).  Never imported by the product package."""
import ctypes as C
import math

import numpy as np

F32 = np.float32
NUM_BINS = 360
BIN_RES = F32(180.0) / F32(NUM_BINS)
DIST_SQ_THRESHOLD = F32((math.sin(float(BIN_RES) / 180.0 * math.pi) * 5.0) ** 2)
FLT_MAX = np.finfo(np.float32).max


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def get_transformation(oracle, pose6):
    m = np.zeros(12, np.float32)
    f = oracle.dll.lvo_test_get_transformation
    f.restype = None
    f.argtypes = [C.c_float] * 6 + [C.c_void_p]
    f(*[float(v) for v in np.asarray(pose6, np.float32)], _p(m))
    return m.reshape(3, 4)


def affine_inverse(M):
    """Eigen::Affine3f::inverse(): cofactor 3x3 inverse (3-term sums as a0 + (a1 + a2)), translation -(inv * t)"""
    m = lambda r, c: F32(M[r, c])  # noqa: E731

    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return F32(m(i1, j1) * m(i2, j2)) - F32(m(i1, j2) * m(i2, j1))
    c0 = [cof(0, 0), cof(1, 0), cof(2, 0)]
    det = c0[0] * m(0, 0) + (c0[1] * m(1, 0) + c0[2] * m(2, 0))
    invdet = F32(1.0) / det
    R = np.zeros((3, 4), np.float32)
    for i in range(3):
        for j in range(3):
            R[i, j] = cof(j, i) * invdet
    for i in range(3):
        R[i, 3] = -(R[i, 0] * m(0, 3) + (R[i, 1] * m(1, 3) + R[i, 2] * m(2, 3)))
    return R


def transform(M, xyzi):
    """pcl::transformPointCloud in the library's order ((m0 x + m1 y) + m2 z) + t, f32"""
    x, y, z = xyzi[:, 0], xyzi[:, 1], xyzi[:, 2]
    o = xyzi.copy()
    for r in range(3):
        o[:, r] = ((F32(M[r, 0]) * x + F32(M[r, 1]) * y) + F32(M[r, 2]) * z) + F32(M[r, 3])
    return o


def roundf(v):
    v = np.asarray(v, np.float64)                       # exact for f32 inputs
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def atan2f(a, b):
    return np.arctan2(np.asarray(a, np.float64), np.asarray(b, np.float64)).astype(np.float32)


def point_distance(p):
    return np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])


def fov_keep(p):
    """lidar_callback's keep test"""
    with np.errstate(all="ignore"):
        return (p[:, 0] >= 0) & (np.abs(p[:, 1] / p[:, 0]) <= 10) & (np.abs(p[:, 2] / p[:, 0]) <= 10)


def bin_angles(p):
    """(row_real, col_real) = row_angle / bin_res and col_angle / bin_res in f32, the values roundf sees"""
    ra = atan2f(p[:, 2], np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]))
    row_angle = (ra.astype(np.float64) * 180.0 / math.pi + 90.0).astype(np.float32)
    ca = atan2f(p[:, 0], p[:, 1])
    col_angle = (ca.astype(np.float64) * 180.0 / math.pi).astype(np.float32)
    return row_angle / BIN_RES, col_angle / BIN_RES


def range_image(local):
    """step 3: per bin the kept cloud index (-1 = empty), [360, 360]"""
    n = len(local)
    with np.errstate(all="ignore"):
        skip = (local[:, 0] < 0) | (np.abs(local[:, 1] / local[:, 0]) > 10) | (np.abs(local[:, 2] / local[:, 0]) > 10)
        rr, cc = bin_angles(local)
        row, col = roundf(rr), roundf(cc)
        dist = point_distance(local)
    ok = ~skip & (row >= 0) & (row < NUM_BINS) & (col >= 0) & (col < NUM_BINS) & (dist < FLT_MAX)
    idx = np.nonzero(ok)[0]
    b = row[idx] * NUM_BINS + col[idx]
    order = np.lexsort((idx, dist[idx], b))            # first point in cloud order wins ties (strict <)
    b, idx = b[order], idx[order]
    first = np.ones(len(b), bool)
    first[1:] = b[1:] != b[:-1]
    sel = np.full(NUM_BINS * NUM_BINS, -1, np.int64)
    sel[b[first]] = idx[first]
    assert n == 0 or sel.max() < n
    return sel.reshape(NUM_BINS, NUM_BINS)


def sphere_cloud(local, sel):
    """steps 4-5: occupied bins in row-major order on the unit sphere, intensity = range"""
    flat = sel.reshape(-1)
    idx = flat[flat >= 0]
    p = local[idx].copy()
    with np.errstate(all="ignore"):
        rng = point_distance(p)
        p[:, 0] /= rng; p[:, 1] /= rng; p[:, 2] /= rng
    p[:, 3] = rng
    return p, idx


def feature_rays(features_xyz):
    """0.5: Eigen normalize() in f32, then ROS axes (z, -x, -y)"""
    f = np.ascontiguousarray(features_xyz, np.float32).reshape(-1, 3)
    sq = f[:, 0] * f[:, 0] + (f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2])
    s = np.sqrt(sq)
    with np.errstate(all="ignore"):
        nrm = np.where((sq > 0)[:, None], f / s[:, None], f)
    return np.stack([nrm[:, 2], -nrm[:, 0], -nrm[:, 1]], 1).astype(np.float32)


def knn3(oracle, sphere, V):
    """KdTreeFLANN nearestKSearch(k = 3), exact and sorted; non-finite sphere points are not in the tree"""
    fin = np.nonzero(np.isfinite(sphere[:, :3]).all(1))[0]
    pts = np.ascontiguousarray(sphere[fin, :3], np.float32)
    q = np.ascontiguousarray(V, np.float32)
    idx = np.full((len(q), 5), -1, np.int32)
    sqd = np.full((len(q), 5), -1.0, np.float32)
    if len(q) and len(pts):
        oracle.dll.lvo_test_kdtree_knn(_p(pts), len(pts), _p(q), len(q), _p(idx), _p(sqd))
    idx3 = np.where(idx[:, :3] >= 0, fin[np.maximum(idx[:, :3], 0)], -1)
    return idx3, sqd[:, :3]


def brute_knn3(sphere, V):
    """exact 3-NN by exhaustive search: f32 squared distances in FLANN's L2_Simple order (dx*dx + dy*dy) + dz*dz, NaN
    distances dropped, ordered by the distance's bits first and the sphere index second; padded with -1 / -1.0"""
    S = np.ascontiguousarray(sphere, np.float32).reshape(len(sphere), -1)[:, :3]
    q = np.ascontiguousarray(V, np.float32).reshape(-1, 3)
    idx = np.full((len(q), 3), -1, np.int32)
    sqd = np.full((len(q), 3), -1.0, np.float32)
    if len(S) == 0 or len(q) == 0:
        return idx, sqd
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    j = np.arange(len(S), dtype=np.uint64)
    step = max(1, (1 << 22) // len(S))
    for b in range(0, len(q), step):
        v = q[b:b + step]
        with np.errstate(all="ignore"):
            dx, dy, dz = (v[:, k, None] - S[None, :, k] for k in range(3))
            d = (dx * dx + dy * dy) + dz * dz
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j[None, :]   # d >= 0: its bits order like its value
        key[np.isnan(d)] = none
        if key.shape[1] < 3:
            key = np.concatenate([key, np.full((len(v), 3 - key.shape[1]), none, np.uint64)], 1)
        best = np.sort(np.partition(key, 2, axis=1)[:, :3], axis=1)
        ok = best != none
        idx[b:b + step] = np.where(ok, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
        sqd[b:b + step] = np.where(ok, (best >> np.uint64(32)).astype(np.uint32).view(np.float32), F32(-1.0))
    return idx, sqd


def accepted(nbr, sqd):
    """step 6's test: three neighbours and the third below the threshold"""
    return (nbr >= 0).all(1) & (sqd[:, 2] < DIST_SQ_THRESHOLD)


def check_search(sphere, V, nbr, sqd, depth, full):
    """a device search (nbr, sqd, depth) against the exhaustive one on the device's own sphere cloud [n, 4].  Full
    search: every neighbour and distance bit.  Band: the same for every feature either side accepts; where both reject,
    the band's third distance is not below the true one.  Every accepted feature's depth is intersect() of the device's
    own neighbours, bit for bit; every other depth is -1.  Returns the accepted mask."""
    V = np.ascontiguousarray(V, np.float32).reshape(-1, 3)
    b_nbr, b_sqd = brute_knn3(sphere, V)
    acc = accepted(nbr, sqd)
    both = acc | accepted(b_nbr, b_sqd)
    must = np.ones(len(V), bool) if full else both
    bad = np.nonzero(must & ((nbr != b_nbr).any(1) | (sqd.view(np.uint32) != b_sqd.view(np.uint32)).any(1)))[0]
    assert len(bad) == 0, (bad[:5], nbr[bad[:5]], b_nbr[bad[:5]], sqd[bad[:5]], b_sqd[bad[:5]])
    third = lambda n, s: np.where(n[:, 2] >= 0, s[:, 2], F32(np.inf))  # noqa: E731   (no third neighbour: beyond any distance)
    assert not (third(nbr, sqd)[~both] < third(b_nbr, b_sqd)[~both]).any()
    want = np.full(len(V), -1.0, np.float32)
    for i in np.nonzero(acc)[0]:
        want[i] = intersect(sphere, nbr[i], V[i])
    assert np.array_equal(depth.view(np.uint32), want.view(np.uint32)), np.nonzero(depth.view(np.uint32) != want.view(np.uint32))[0][:5]
    return acc


def intersect(sphere, nbr, V):
    """step 7 for one feature whose 3 neighbours were accepted: the published depth (> 3.0, else -1)"""
    P = [sphere[k] for k in nbr]
    r = [F32(p[3]) for p in P]
    A, B, Cc = [np.array([F32(p[0]) * rr, F32(p[1]) * rr, F32(p[2]) * rr], np.float32) for p, rr in zip(P, r)]
    u, w = (A - B).astype(np.float32), (B - Cc).astype(np.float32)
    N = np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]], np.float32)
    v = V.astype(np.float32)
    with np.errstate(all="ignore"):
        s = F32((N[0] * A[0] + N[1] * A[1]) + N[2] * A[2]) / F32((N[0] * v[0] + N[1] * v[1]) + N[2] * v[2])
    mn, mx = min(r[0], min(r[1], r[2])), max(r[0], max(r[1], r[2]))
    if F32(mx - mn) > 2 or s <= 0.5:
        return F32(-1.0)
    if F32(s - mx) > 0:
        s = mx
    elif F32(s - mn) < 0:
        s = mn
    d = F32(v[0] * s)
    return d if d > 3.0 else F32(-1.0)


def get_depth(oracle, depth_cloud, pose6, features_xyz):
    """DepthRegister::get_depth -> (depth [n], debug dict: local, sel, sphere, sphere_idx, nbr, sqd)"""
    f = np.ascontiguousarray(features_xyz, np.float32).reshape(-1, 3)
    out = np.full(len(f), -1.0, np.float32)
    dbg = {}
    cloud = np.ascontiguousarray(depth_cloud, np.float32).reshape(-1, 4)
    if pose6 is None or len(cloud) == 0 or len(f) == 0:
        return out, dbg
    Minv = affine_inverse(get_transformation(oracle, pose6))
    local = transform(Minv, cloud)
    sel = range_image(local)
    sphere, sidx = sphere_cloud(local, sel)
    V = feature_rays(f)
    dbg.update(local=local, sel=sel, sphere=sphere, sphere_idx=sidx, V=V)
    if len(sphere) < 10:
        return out, dbg
    nbr, sqd = knn3(oracle, sphere, V)
    dbg.update(nbr=nbr, sqd=sqd)
    for i in range(len(f)):
        if (nbr[i] >= 0).all() and sqd[i, 2] < DIST_SQ_THRESHOLD:
            out[i] = intersect(sphere, nbr[i], V[i])
    return out, dbg


class Window:
    """lidar_callback: skip counting, VoxelGrid 0.2, field of view, world frame, 5 s queue, fused VoxelGrid 0.2"""

    def __init__(self, pkg, oracle, lidar_skip=3, window_s=5.0):
        self.pkg, self.oracle = pkg, oracle
        self.h = pkg.LidarHotpath(oracle, max_raw_points=1 << 21, max_map_points=1 << 21)
        self.skip, self.window = int(lidar_skip), float(window_s)
        self.lidar_count = -1
        self.clouds, self.stamps = [], []
        self.depth_cloud = np.zeros((0, 4), np.float32)
        self.cells = self.counts = None

    def voxel(self, xyzi):
        out = self.h.voxel_downsample(xyzi, 0.2)
        return self.pkg._abi.pts_xyzi(out).copy() if len(out) else np.zeros((0, 4), np.float32)

    def lidar_callback(self, cloud, pose6, stamp):
        self.lidar_count += 1
        if self.lidar_count % (self.skip + 1) != 0:
            return False
        if pose6 is None:
            return False
        ds = self.voxel(np.ascontiguousarray(cloud, np.float32).reshape(-1, 4))
        ds = ds[fov_keep(ds)]
        M = get_transformation(self.oracle, pose6)
        glob = transform(M, ds)
        self.clouds.append(glob); self.stamps.append(float(stamp))
        while self.stamps and float(stamp) - self.stamps[0] > self.window:
            self.clouds.pop(0); self.stamps.pop(0)
        fused = np.concatenate(self.clouds) if self.clouds else np.zeros((0, 4), np.float32)
        self.depth_cloud = self.voxel(fused)
        A = self.pkg._abi
        self.cells = self.h.debug_get(A.DBG_VOXEL_CELLS, np.int32) if len(fused) else np.zeros(0, np.int32)
        self.counts = self.h.debug_get(A.DBG_VOXEL_COUNTS, np.int32) if len(fused) else np.zeros(0, np.int32)
        return True
