"""TEST INFRASTRUCTURE — restatement of mapOptimization's global map (include/lvi_gmap.h).

fuse()          the fused clouds of publishGlobalMap (corner_k then surf_k per key, mapOptimization.cpp:496-501) and of
                save_map (corner and surf separately, :193-200): every key cloud through the oracle's lvi_transform_cloud
                with the key's pose, in list order, duplicates included
voxel()         the VoxelGrid of that cloud: PCL's overflow rule (centroid_ref.pcl_overflow: output = input), else the
                cells, counts and order of the oracle's lvi_voxel_downsample and the centroids of centroid_ref.model_centroids
voxel_cells()   the same cells and counts in numpy (multi-million-point clouds, where the oracle and the model are slow)
select_keys()   publishGlobalMap's key selection (:470-495, steps 2-6 of DESIGN §12) in numpy, the key-pose VoxelGrid
                through a caller-given filter (the oracle's)

Never imported by the product package."""
import numpy as np

import centroid_ref as R

F32 = np.float32
CORNER, SURF, CORNER_SURF = 0, 1, 2


def fuse(o, corners, surfs, poses, keys, which):
    """o: an oracle LidarHotpath; corners / surfs / poses indexed by key"""
    parts = []
    for k in keys:
        if which in (CORNER, CORNER_SURF):
            parts.append(o.transform_cloud(corners[k], poses[k]))
        if which in (SURF, CORNER_SURF):
            parts.append(o.transform_cloud(surfs[k], poses[k]))
    if not parts:
        return np.zeros(0, corners[0].dtype)
    return np.concatenate(parts)


def xyzi(pts):
    return np.ascontiguousarray(pts).view(F32).reshape(-1, 4)


def voxel(pkg, o, pts, leaf, centroids=True):
    """dict(overflow, cells, counts, pts): the filter's output for `pts` (PT_DTYPE) at `leaf`"""
    p = xyzi(pts)
    if R.pcl_overflow(p[:, :3], leaf):
        return dict(overflow=True, cells=None, counts=None, pts=p.copy())
    o.voxel_downsample(pts, leaf)
    cells = o.debug_get(pkg._abi.DBG_VOXEL_CELLS, np.int32)
    counts = o.debug_get(pkg._abi.DBG_VOXEL_COUNTS, np.int32)
    out = R.model_centroids(p, leaf)["pts"] if centroids else None
    return dict(overflow=False, cells=cells, counts=counts, pts=out)


def voxel_cells(pts, leaf):
    """PCL's linear voxel idx in output order, points per voxel, and the float64 mean of every voxel (numpy)"""
    p = xyzi(pts)
    c = R.pcl_cells(p[:, :3], leaf)
    mn = c.min(axis=0)
    div = c.max(axis=0) - mn + 1
    idx = (c[:, 0] - mn[0]) + (c[:, 1] - mn[1]) * div[0] + (c[:, 2] - mn[2]) * div[0] * div[1]
    order = np.argsort(idx, kind="stable")
    si = idx[order]
    head = np.ones(len(si), bool)
    head[1:] = si[1:] != si[:-1]
    starts = np.nonzero(head)[0]
    counts = np.diff(np.append(starts, len(si)))
    mean = np.add.reduceat(p[order].astype(np.float64), starts, axis=0) / counts[:, None]
    return si[starts].astype(np.int64), counts.astype(np.int64), mean


def _sqd(a, b):
    """(dx*dx + dy*dy) + dz*dz in f32 (pcl's squared distance, the host mirror's keyPoseSqDist)"""
    a = np.asarray(a, F32).reshape(-1, 4)
    dx, dy, dz = (a[:, 0] - F32(b[0])), (a[:, 1] - F32(b[1])), (a[:, 2] - F32(b[2]))
    return (dx * dx + dy * dy) + dz * dz


def select_keys(poses3d, radius, density, voxel_filter):
    """steps 2-6: poses3d [n, 4] f32 (x, y, z, index) = cloudKeyPoses3D; voxel_filter(pts [m, 4] f32, leaf) -> DS poses
    [k, 4] f32 in PCL's order.  Returns the key list of globalMapKeyFrames' fuse (a key may appear twice)."""
    P = np.ascontiguousarray(poses3d, F32).reshape(-1, 4)
    if len(P) == 0:
        return np.zeros(0, np.int32)
    back = P[-1]
    R2 = float(F32(radius)) ** 2
    d = _sqd(P, back)
    hit = np.nonzero(d.astype(np.float64) <= R2)[0]
    near = P[hit[np.argsort(d[hit], kind="stable")]]              # radiusSearch: by distance, ties by index
    ds = np.asarray(voxel_filter(near, F32(density)), F32).reshape(-1, 4).copy()
    keys = []
    for pt in ds:
        best = int(np.argmin(_sqd(P, pt)))                          # nearestKSearch(pt, 1): first index on ties
        if np.sqrt(_sqd(pt[None, :], back)[0]) > F32(radius):       # pointDistance of the DS centroid to back()
            continue
        keys.append(int(P[best, 3]))
    return np.asarray(keys, np.int32)
