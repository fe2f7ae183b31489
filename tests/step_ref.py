"""float64 reference of the end of ONE Gauss-Newton iteration (LMOptimization past the row products,
mapOptimization.cpp:1210-1311): sums in, pose increment out.  numpy only: neither the product nor the
oracle is imported here, so both can be measured against it.

One record = 27 floats: the 21 upper-triangular entries of AtA row by row, then the 6 of AtB (LVI_DBG_ICP_JTJ)."""
from collections import namedtuple

import numpy as np

EIG_THRESHOLD = 100.0          # eignThre (:1275)
RAD2DEG = 57.29578             # pcl::rad2deg(float)

Step = namedtuple("Step", "step eigenvalues degenerate converged proj_gap X delta_r delta_t")


def tri_index(r, c):
    """position of AtA[r][c] (r <= c) in the record: k = r*6 - r(r-1)/2 + (c-r)"""
    return r * 6 - (r * (r - 1)) // 2 + (c - r)


def unpack(rec):
    rec = np.asarray(rec, np.float64).reshape(27)
    A = np.zeros((6, 6))
    for r in range(6):
        for c in range(r, 6):
            A[r, c] = A[c, r] = rec[tri_index(r, c)]
    return A, rec[21:27].copy()


def pack(A, b):
    A = np.asarray(A, np.float64)
    return np.array([A[r, c] for r in range(6) for c in range(r, 6)] + list(np.asarray(b, np.float64)))


def eigenvalues(rec):
    return np.linalg.eigvalsh(unpack(rec)[0])


def projector(rec):
    """matP = V^-1 V2 of iteration 0: the orthogonal projector onto the eigenvectors whose eigenvalue is >= 100"""
    w, V = np.linalg.eigh(unpack(rec)[0])                  # ascending, eigenvectors in columns
    keep = V[:, w >= EIG_THRESHOLD]
    return keep @ keep.T, w


def gn_step(rec, iteration, degenerate_in=False):
    """the step the reference adds to transformTobeMapped at the end of iteration `iteration`.
    degenerate_in: isDegenerate as iteration 0 of the same frame left it (ignored on iteration 0, which decides it)."""
    A, b = unpack(rec)
    try:
        X = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:                          # cv::solve returns false and zeroes dst
        X = np.zeros(6)
    w = np.linalg.eigvalsh(A)
    if iteration == 0:
        P, w = projector(rec)
        degenerate = bool((w < EIG_THRESHOLD).any())
        step = P @ X if degenerate else X
    else:
        degenerate = bool(degenerate_in)
        step = np.zeros(6) if degenerate else X            # the local matP shadows the member: all zeros here
        P = np.zeros((6, 6)) if degenerate else np.eye(6)
    gap = float(np.abs(X - P @ X).max()) if degenerate else 0.0
    dR = float(np.linalg.norm(step[:3] * RAD2DEG))
    dT = float(np.linalg.norm(step[3:] * 100.0))
    return Step(step, w, degenerate, dR < 0.05 and dT < 0.05, gap, X, dR, dT)


def replay(jtj, break_enabled=True):
    """every recorded iteration of one frame: [Step per iteration], degenerate, converged, iters the loop should have run.
    jtj: f32[iters*27].  `iters` is the number of iterations the reference's loop runs given these steps: up to the first
    converged one with the break enabled, all recorded ones otherwise."""
    recs = np.asarray(jtj, np.float64).reshape(-1, 27)
    steps, degenerate, converged, iters = [], False, False, len(recs)
    for i, rec in enumerate(recs):
        s = gn_step(rec, i, degenerate)
        if i == 0:
            degenerate = s.degenerate
        steps.append(s)
        if s.converged and not converged:
            converged = True
            if break_enabled:
                iters = i + 1
    return steps, degenerate, converged, iters


def f32_spacing(x):
    """distance between neighbouring float32 numbers at magnitude |x|"""
    return float(np.spacing(np.float32(abs(float(x)))))


def normal_sums(ori, coeff, pose):
    """AtA and AtB of one iteration in float64 from its selected rows (mapOptimization.cpp:1225-1245): ori [n,3] the
    selected scan points (sensor frame), coeff [n,4] their coefficients (x, y, z, intensity), pose the pose the rows
    belong to.  Returns (sums[27], terms[27]): the record, and the sum of the absolute values of each entry's terms."""
    ori, coeff = np.asarray(ori, np.float64), np.asarray(coeff, np.float64)
    T = np.asarray(pose, np.float32).astype(np.float64)
    srx, crx, sry, cry, srz, crz = np.sin(T[1]), np.cos(T[1]), np.sin(T[2]), np.cos(T[2]), np.sin(T[0]), np.cos(T[0])
    px, py, pz = ori[:, 1], ori[:, 2], ori[:, 0]                   # lidar -> camera (:1227-1234)
    cx, cy, cz = coeff[:, 1], coeff[:, 2], coeff[:, 0]
    arx = ((crx * sry * srz * px + crx * crz * sry * py - srx * sry * pz) * cx
           + (-srx * srz * px - crz * srx * py - crx * pz) * cy
           + (crx * cry * srz * px + crx * cry * crz * py - cry * srx * pz) * cz)
    ary = (((cry * srx * srz - crz * sry) * px + (sry * srz + cry * crz * srx) * py + crx * cry * pz) * cx
           + ((-cry * crz - srx * sry * srz) * px + (cry * srz - crz * srx * sry) * py - crx * sry * pz) * cz)
    arz = (((crz * srx * sry - cry * srz) * px + (-cry * crz - srx * sry * srz) * py) * cx
           + (crx * crz * px - crx * srz * py) * cy
           + ((sry * srz + cry * crz * srx) * px + (crz * sry - cry * srx * srz) * py) * cz)
    A = np.stack([arz, arx, ary, cz, cx, cy], 1)
    b = -coeff[:, 3]
    sums, terms = np.zeros(27), np.zeros(27)
    for r in range(6):
        for c in range(r, 6):
            t = A[:, r] * A[:, c]
            sums[tri_index(r, c)], terms[tri_index(r, c)] = t.sum(), np.abs(t).sum()
        t = A[:, r] * b
        sums[21 + r], terms[21 + r] = t.sum(), np.abs(t).sum()
    return sums, terms
