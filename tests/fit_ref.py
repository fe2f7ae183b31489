"""float64 reference of the per-feature coefficients of scan-to-map Gauss-Newton: cornerOptimization's line through five
neighbours and its eigenvalue gate (mapOptimization.cpp:1006-1096), surfOptimization's plane through five neighbours and its
0.2 m gate (:1098-1167).  numpy only: neither the product nor the oracle is imported here, so both can be measured against it.

Every function works on N features at once.  The inputs are float32 VALUES read as float64 (the five neighbours as the map
holds them, the feature in the map frame, the feature's sensor-frame point); everything after that is float64, so the result
is what the reference's formulas give on exactly those numbers before any float32 rounding of the decompositions.

The plane solve has the semantics of Eigen's `colPivHouseholderQr().solve` (3.3 / 3.4): pivoting on the largest remaining
column norm, nonzeroPivots() decided by `threshold_helper = (max column norm * epsilon)^2 / rows` with the FLOAT32 epsilon
(the decision the reference takes is a float32 one), a dropped column's component zero: the basic solution, not the
minimum-norm one of numpy's lstsq."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
RATIO_GATE = 3.0                # matD1[0] > 3 * matD1[1]   (:1052)
PLANE_GATE = 0.2                # fabs(pa x + pb y + pc z + pd) > 0.2 rejects   (:1140)
S_GATE = 0.1                    # s > 0.1   (:1084, :1155)
NEAR_GATE = 1.0                 # pointSearchSqDis[4] < 1.0   (:1025, :1121)


def f32_spacing(x):
    """distance between neighbouring float32 numbers at magnitude |x|"""
    return float(np.spacing(np.float32(abs(float(x)))))


# ----------------------------------------------------------------------------- pointAssociateToMap
def pose_matrix_f32(pose):
    """pcl::getTransformation(x, y, z, roll, pitch, yaw) in float32 (PCL common/eigen.hpp): rows of the 3x4 matrix.
    pose = [roll, pitch, yaw, x, y, z] (trans2Affine3f, :404-407)"""
    f = np.float32
    T = np.asarray(pose, f)
    roll, pitch, yaw, x, y, z = (f(v) for v in T)
    A, B, C, D, E, F = f(np.cos(yaw)), f(np.sin(yaw)), f(np.cos(pitch)), f(np.sin(pitch)), f(np.cos(roll)), f(np.sin(roll))
    DE, DF = f(D * E), f(D * F)
    return np.array([[f(A * C), f(f(A * DF) - f(B * E)), f(f(B * F) + f(A * DE)), x],
                     [f(B * C), f(f(A * E) + f(B * DF)), f(f(B * DE) - f(A * F)), y],
                     [f(-D), f(C * F), f(C * E), z]], f)


def to_map(pose, pts):
    """pointAssociateToMap (:339-345) in float32, one rounding per operation, left to right: [n, 3] float32"""
    M = pose_matrix_f32(pose)
    p = np.asarray(pts, np.float32)[:, :3]
    out = np.empty((len(p), 3), np.float32)
    for r in range(3):
        acc = (M[r, 0] * p[:, 0]).astype(np.float32)
        acc = (acc + (M[r, 1] * p[:, 1]).astype(np.float32)).astype(np.float32)
        acc = (acc + (M[r, 2] * p[:, 2]).astype(np.float32)).astype(np.float32)
        out[:, r] = (acc + M[r, 3]).astype(np.float32)
    return out


# ----------------------------------------------------------------------------- the corner line
def corner(nb, sel, sqd4=None):
    """nb [N,5,3], sel [N,3] (map frame), sqd4 [N] the squared distance of the fifth neighbour (None: inside the 1 m gate).
    Returns a dict of arrays: centroid, eigenvalues (descending), ratio, direction (unit, sign arbitrary), p1 / p2, la lb lc
    ld2 s, coeff [N,4], flag, and the margins m_ratio, m_s, m_near."""
    nb, sel = np.asarray(nb, np.float64), np.asarray(sel, np.float64)
    N = len(nb)
    c = nb.sum(1) / 5.0
    d = nb - c[:, None, :]
    cov = np.einsum("nij,nik->njk", d, d) / 5.0
    w, V = np.linalg.eigh(cov)                                    # ascending
    lam = np.maximum(w[:, ::-1], 0.0)                             # an exactly singular covariance may come back as -1e-20
    v = V[:, :, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(lam[:, 1] > 0, lam[:, 0] / lam[:, 1], np.inf)
    p1, p2 = c + 0.1 * v, c - 0.1 * v
    x0, y0, z0 = sel.T
    x1, y1, z1 = p1.T
    x2, y2, z2 = p2.T
    m11 = (x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)
    m12 = (x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1)
    m13 = (y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1)
    a012 = np.sqrt(m11 * m11 + m12 * m12 + m13 * m13)
    l12 = np.sqrt((x1 - x2) ** 2 + (y1 - y2) ** 2 + (z1 - z2) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        la = ((y1 - y2) * m11 + (z1 - z2) * m12) / a012 / l12
        lb = -((x1 - x2) * m11 - (z1 - z2) * m13) / a012 / l12
        lc = -((x1 - x2) * m12 + (y1 - y2) * m13) / a012 / l12
        ld2 = a012 / l12
    s = 1 - 0.9 * np.abs(ld2)
    coeff = np.stack([s * la, s * lb, s * lc, s * ld2], 1)
    sqd4 = np.zeros(N) if sqd4 is None else np.asarray(sqd4, np.float64)
    near = sqd4 < NEAR_GATE
    flag = near & (lam[:, 0] > RATIO_GATE * lam[:, 1]) & (s > S_GATE)
    with np.errstate(invalid="ignore"):
        m_ratio = np.where(np.isfinite(ratio), np.abs(ratio - RATIO_GATE) / RATIO_GATE, np.inf)
    return dict(centroid=c, eigenvalues=lam, ratio=ratio, direction=v, p1=p1, p2=p2, la=la, lb=lb, lc=lc, ld2=ld2, s=s,
                coeff=coeff, flag=flag, near=near, m_ratio=m_ratio, m_s=np.abs(s - S_GATE), m_near=np.abs(sqd4 - NEAR_GATE))


# ----------------------------------------------------------------------------- the surf plane
def colpiv_solve(A, b):
    """x of A x = b, A [N,5,3], b [N,5], as Eigen's ColPivHouseholderQR<Matrix<float,5,3>>::solve decides it, in float64.
    Returns x [N,3], rank [N], rank_near [N] (a rank decision within a factor 10 of its threshold, in norms), pivot_tied [N]
    (two candidate pivot columns within 1e-3 of each other in norm while the system is rank deficient: which column is
    dropped is then a rounding accident)."""
    A = np.array(A, np.float64)
    b = np.array(b, np.float64)
    N, rows, cols = A.shape
    ar = np.arange(N)
    perm = np.tile(np.arange(cols), (N, 1))
    thr = (np.sqrt((A * A).sum(1)).max(1) * EPS32) ** 2 / rows
    rank = np.full(N, cols)
    rank_near = np.zeros(N, bool)
    tie_seen = np.zeros(N, bool)
    tiny = np.finfo(np.float64).tiny
    for k in range(cols):
        sq = (A[:, k:, :] ** 2).sum(1)
        sq[:, :k] = -1.0
        big = sq.argmax(1)
        bigsq = sq[ar, big]
        srt = np.sort(sq[:, k:], 1)
        if cols - k > 1:
            tie_seen |= np.sqrt(srt[:, -2]) >= (1 - 1e-3) * np.sqrt(srt[:, -1])
        undecided = rank == cols
        lim = thr * (rows - k)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(lim > 0, bigsq / lim, np.inf)
        rank_near |= undecided & (q >= 1e-2) & (q <= 1e2)          # a factor 10 in norms = 100 in squared norms
        rank = np.where(undecided & (bigsq < lim), k, rank)
        # swap columns k and big
        ck, cb = A[ar, :, k].copy(), A[ar, :, big].copy()
        A[ar, :, k], A[ar, :, big] = cb, ck
        pk, pb = perm[ar, k].copy(), perm[ar, big].copy()
        perm[ar, k], perm[ar, big] = pb, pk
        # makeHouseholderInPlace
        c0 = A[:, k, k].copy()
        tail = (A[:, k + 1:, k] ** 2).sum(1)
        flat = tail <= tiny
        beta = np.where(c0 >= 0, -1.0, 1.0) * np.sqrt(c0 * c0 + tail)
        beta = np.where(flat, c0, beta)
        with np.errstate(divide="ignore", invalid="ignore"):
            ess = np.where(flat[:, None], 0.0, A[:, k + 1:, k] / np.where(flat, 1.0, c0 - beta)[:, None])
            tau = np.where(flat, 0.0, (beta - c0) / np.where(flat, 1.0, beta))
        A[:, k + 1:, k] = ess
        A[:, k, k] = beta
        for j in range(k + 1, cols):
            sdot = ((ess * A[:, k + 1:, j]).sum(1) + A[:, k, j]) * tau
            A[:, k, j] -= sdot
            A[:, k + 1:, j] -= sdot[:, None] * ess
        sdot = ((ess * b[:, k + 1:]).sum(1) + b[:, k]) * tau
        b[:, k] -= sdot
        b[:, k + 1:] -= sdot[:, None] * ess
    y = np.zeros((N, cols))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(cols - 1, -1, -1):
            acc = b[:, i].copy()
            for j in range(i + 1, cols):
                acc -= A[:, i, j] * y[:, j]
            y[:, i] = np.where(i < rank, acc / A[:, i, i], 0.0)
    x = np.zeros((N, cols))
    for i in range(cols):
        x[ar, perm[:, i]] = y[:, i]
    return x, rank, rank_near, tie_seen & (rank < cols)


def surf(nb, sel, ori, sqd4=None):
    """nb [N,5,3], sel [N,3] (map frame), ori [N,3] (sensor frame).  Returns a dict of arrays: x (the solution of A x = -1),
    rank, normal, pd, maxdist, pd2, s, coeff [N,4], flag, cond, rank_near / pivot_tied, and the margins m_plane, m_s, m_near."""
    nb, sel, ori = np.asarray(nb, np.float64), np.asarray(sel, np.float64), np.asarray(ori, np.float64)
    N = len(nb)
    x, rank, rank_near, pivot_tied = colpiv_solve(nb, -np.ones((N, 5)))
    with np.errstate(divide="ignore", invalid="ignore"):
        ps = np.sqrt((x * x).sum(1))
        n = x / ps[:, None]
        pd = 1.0 / ps
        dist = np.abs(np.einsum("nij,nj->ni", nb, n) + pd[:, None])
        maxdist = dist.max(1)
        pd2 = (n * sel).sum(1) + pd
        s = 1 - 0.9 * np.abs(pd2) / np.sqrt(np.sqrt((ori * ori).sum(1)))
        coeff = np.concatenate([s[:, None] * n, (s * pd2)[:, None]], 1)
        sqd4 = np.zeros(N) if sqd4 is None else np.asarray(sqd4, np.float64)
        near = sqd4 < NEAR_GATE
        flag = near & (maxdist <= PLANE_GATE) & (s > S_GATE)          # NaN (x = 0) compares false, as in the reference
        sv = np.linalg.svd(nb, compute_uv=False)
        cond = np.where(sv[:, 2] > 0, sv[:, 0] / sv[:, 2], np.inf)
    return dict(x=x, rank=rank, normal=n, pd=pd, maxdist=maxdist, pd2=pd2, s=s, coeff=coeff, flag=flag, near=near, cond=cond,
                rank_near=rank_near, pivot_tied=pivot_tied, m_plane=np.abs(maxdist - PLANE_GATE), m_s=np.abs(s - S_GATE),
                m_near=np.abs(sqd4 - NEAR_GATE))


# ----------------------------------------------------------------------------- decidability, errors
def decidable(res, which, margin=1e-3):
    """every gate of the feature keeps `margin` from its threshold and the rank decision is not a rounding accident.  A gate
    behind a failed earlier gate does not count: a rejected plane's s, or anything past a fifth neighbour beyond 1 m."""
    ok = res["m_near"] >= margin
    inside = res["near"]
    if which == 0:
        first = res["m_ratio"] >= margin
        passed = res["eigenvalues"][:, 0] > RATIO_GATE * res["eigenvalues"][:, 1]
    else:
        with np.errstate(invalid="ignore"):
            first = (res["m_plane"] >= margin) & ~res["rank_near"] & ~res["pivot_tied"]
            passed = res["maxdist"] <= PLANE_GATE
    with np.errstate(invalid="ignore"):
        second = res["m_s"] >= margin
    return ok & (~inside | (first & (~passed | second)))


def coeff_errors(coeff, res):
    """max |coeff - coeff64| per feature, direction part (x, y, z) and distance part (intensity) apart"""
    d = np.abs(np.asarray(coeff, np.float64) - res["coeff"])
    return d[:, :3].max(1), d[:, 3]
