"""Host restatement of include/lvi_fmat.h: OpenCV 4.5.x cv::findFundamentalMat(pts1, pts2, FM_RANSAC, thr,
confidence, maxIters=1000, mask) as rejectWithF calls it (feature_tracker.cpp:229).

Scalar Python for the integer sample stream and the 7-point kernel (the kernel's operation order, so the same inputs give
the same bits wherever the host and device libm agree), numpy float64 for the errors.  `find` returns the status and a
trace shaped like FundamentalRansac.trace() plus the walk's info, so tests compare the two call for call."""
import math
import struct

import numpy as np

MODEL_POINTS = 7
RANSAC_MAX_ATTEMPTS = 10000
LMEDS_MAX_ATTEMPTS = 1000
LMEDS_OUTLIER_RATIO = 0.45
FLT_EPSILON = 2.0 ** -23
DBL_EPSILON = 2.0 ** -52
DBL_MIN = 2.2250738585072014e-308
DBL_MAX = 1.7976931348623157e308
M64, M32 = (1 << 64) - 1, (1 << 32) - 1
RNG_COEFF = 4164903690


class CvRng:
    """cv::RNG: multiply-with-carry on a 64-bit state, seeded with (uint64)-1"""

    def __init__(self, state=M64):
        self.s = state & M64

    def next(self):
        self.s = ((self.s & M32) * RNG_COEFF + (self.s >> 32)) & M64
        return self.s & M32

    def uniform(self, a, b):
        return a if a == b else (self.next() % (b - a) + a)


def _f32(v):
    return float(np.float32(v))


def have_collinear(xy):
    """haveCollinearPoints(ms, 7): the last point against every pair of earlier ones; differences in f32"""
    i = MODEL_POINTS - 1
    X = [np.float32(p[0]) for p in xy]
    Y = [np.float32(p[1]) for p in xy]
    for j in range(i):
        dx1, dy1 = float(X[j] - X[i]), float(Y[j] - Y[i])
        for k in range(j):
            dx2, dy2 = float(X[k] - X[i]), float(Y[k] - Y[i])
            if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


def get_subset(rng, p1, p2, n, check, max_attempts, attempts=None):
    """getSubset: draw 7 distinct indices (redrawing duplicates), then checkSubset; None after max_attempts rejections.
    attempts: a one-element list that counts the subsets drawn"""
    for _ in range(max_attempts):
        if attempts is not None:
            attempts[0] += 1
        idx = []
        for _i in range(MODEL_POINTS):
            k = rng.uniform(0, n)
            while k in idx:
                k = rng.uniform(0, n)
            idx.append(k)
        if not check or (not have_collinear(p1[idx]) and not have_collinear(p2[idx])):
            return idx
    return None


def update_num_iters(p, ep, model_points, max_iters):
    """RANSACUpdateNumIters (ptsetreg.cpp)"""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - math.pow(1.0 - ep, model_points)
    if denom < DBL_MIN:
        return 0
    num = math.log(num)
    denom = math.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * (-denom) else int(round(num / denom))


def null_space(A):
    """the kernel's 2-D null space of the 7x9 system: Gauss-Jordan with partial pivoting (first largest |pivot|), a column
    whose largest remaining |entry| is 0 is free; basis k has x[free_k] = 1.  None when the rank is below 7."""
    a = [list(map(float, row)) for row in A]
    piv = []
    r = 0
    for c in range(9):
        if r == 7:
            break
        p, best = r, abs(a[r][c])
        for i in range(r + 1, 7):
            if abs(a[i][c]) > best:
                best, p = abs(a[i][c]), i
        if best == 0:
            continue
        if p != r:
            a[r], a[p] = a[p], a[r]
        new = [row[:] for row in a]
        for i in range(7):
            if i == r:
                continue
            f = a[i][c] / a[r][c]
            new[i][c] = 0.0
            for j in range(c + 1, 9):
                new[i][j] = a[i][j] - f * a[r][j]
        a = new
        piv.append(c)
        r += 1
    if r < 7:
        return None
    free = [c for c in range(9) if c not in piv][:2]
    f1, f2 = [0.0] * 9, [0.0] * 9
    f1[free[0]] = 1.0
    f2[free[1]] = 1.0
    for q in range(7):
        d = a[q][piv[q]]
        f1[piv[q]] = -a[q][free[0]] / d
        f2[piv[q]] = -a[q][free[1]] / d
    return f1, f2


NAN = float("nan")


# C semantics for the cubic's library calls and divisions (NaN / inf instead of Python exceptions)
def _sqrt(x):
    return math.sqrt(x) if x >= 0 else NAN


def _acos(x):
    return math.acos(x) if -1.0 <= x <= 1.0 else NAN


def _cos(x):
    return math.cos(x) if math.isfinite(x) else NAN


def _pow(x, y):
    try:
        return math.pow(x, y)
    except (ValueError, OverflowError):
        return float(np.power(np.float64(x), np.float64(y)))


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def solve_cubic(c):
    """cv::solveCubic (mathfuncs.cpp, 4.x) for c0 x^3 + c1 x^2 + c2 x + c3 -> (n, [x0, x1, x2])"""
    a0, a1, a2, a3 = map(float, c)
    x0 = x1 = x2 = 0.0
    n = 0
    if a0 == 0:
        if a1 == 0:
            if a2 == 0:
                n = -1 if a3 == 0 else 0
            else:
                x0, n = _div(-a3, a2), 1
        else:
            d = a2 * a2 - 4 * a1 * a3
            if d >= 0:
                d = _sqrt(d)
                q1 = (-a2 + d) * 0.5
                q2 = (a2 + d) * -0.5
                if abs(q1) > abs(q2):
                    x0, x1 = _div(q1, a1), _div(a3, q1)
                else:
                    x0, x1 = _div(q2, a1), _div(a3, q2)
                n = 2 if d > 0 else 1
    else:
        a0 = 1.0 / a0
        a1 *= a0
        a2 *= a0
        a3 *= a0
        Q = (a1 * a1 - 3 * a2) * (1.0 / 9)
        R = (a1 * (2 * a1 * a1 - 9 * a2) + 27 * a3) * (1.0 / 54)
        Qcubed = Q * Q * Q
        d = (a1 * a1 * (a2 * a2 - 4 * a1 * a3) + 2 * a2 * (9 * a1 * a3 - 2 * a2 * a2) - 27 * a3 * a3) * (1.0 / 108)
        if d > 0:
            theta = _acos(_div(R, _sqrt(Qcubed)))
            sqrtQ = _sqrt(Q)
            t0 = -2 * sqrtQ
            t1 = theta * (1.0 / 3)
            tpt = 2.0943951023931954923084289221863
            x0 = t0 * _cos(t1) - a1 * (1.0 / 3)
            x1 = t0 * _cos(t1 + tpt) - a1 * (1.0 / 3)
            x2 = t0 * _cos(t1 - tpt) - a1 * (1.0 / 3)
            n = 3
        elif d == 0:
            if R >= 0:
                x0 = -2 * _pow(R, 1.0 / 3) - a1 / 3
                x1 = _pow(R, 1.0 / 3) - a1 / 3
            else:
                x0 = 2 * _pow(-R, 1.0 / 3) - a1 / 3
                x1 = -_pow(-R, 1.0 / 3) - a1 / 3
            x2 = 0.0
            n = 1 if x0 == x1 else 2
            x1 = 0.0 if x0 == x1 else x1
        else:
            d = _sqrt(-d)
            e = _pow(d + abs(R), 1.0 / 3)
            if R > 0:
                e = -e
            x0 = (e + _div(Q, e)) - a1 * (1.0 / 3)
            n = 1
    return n, [x0, x1, x2]


def system(p1, p2):
    """run7Point's rows: (m2, 1)' F (m1, 1) = 0"""
    A = []
    for i in range(7):
        x0, y0 = float(p1[i][0]), float(p1[i][1])
        x1, y1 = float(p2[i][0]), float(p2[i][1])
        A.append([x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, 1.0])
    return A


def run7point(p1, p2, with_roots=False):
    """the 7-point kernel on 7 correspondences -> list of 0..3 F as flat lists of 9 (with_roots: also the roots and the
    basis (f1 - f2, f2) they combine)"""
    ns = null_space(system(p1, p2))
    if ns is None:
        return ([], [], None, None) if with_roots else []
    f1, f2 = ns
    f1 = [f1[i] - f2[i] for i in range(9)]
    t0 = f2[4] * f2[8] - f2[5] * f2[7]
    t1 = f2[3] * f2[8] - f2[5] * f2[6]
    t2 = f2[3] * f2[7] - f2[4] * f2[6]
    c3 = f2[0] * t0 - f2[1] * t1 + f2[2] * t2
    c2 = (f1[0] * t0 - f1[1] * t1 + f1[2] * t2 -
          f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) +
          f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) -
          f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) +
          f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) -
          f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
          f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]))
    t0 = f1[4] * f1[8] - f1[5] * f1[7]
    t1 = f1[3] * f1[8] - f1[5] * f1[6]
    t2 = f1[3] * f1[7] - f1[4] * f1[6]
    c1 = (f2[0] * t0 - f2[1] * t1 + f2[2] * t2 -
          f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) +
          f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) -
          f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) +
          f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) -
          f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
          f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]))
    c0 = f1[0] * t0 - f1[1] * t1 + f1[2] * t2
    n, r = solve_cubic([c0, c1, c2, c3])
    if n < 1 or n > 3:
        return ([], [], f1, f2) if with_roots else []
    out = [combine(f1, f2, r[k]) for k in range(n)]
    return (out, r[:n], f1, f2) if with_roots else out


def combine(f1, f2, root):
    """run7Point's F for one root, normalised to F33 = 1 unless |s| <= DBL_EPSILON"""
    if True:
        lam, mu = root, 1.0
        s = f1[8] * root + f2[8]
        F = [0.0] * 9
        if abs(s) > DBL_EPSILON:
            mu = 1.0 / s
            lam *= mu
            F[8] = 1.0
        for i in range(8):
            F[i] = f1[i] * lam + f2[i] * mu
    return F


def errors(F, p1, p2):
    """FMEstimatorCallback::computeError in float64, OpenCV's order -> f32 errors"""
    F = [float(v) for v in np.asarray(F, np.float64).reshape(9)]
    x1, y1 = p1[:, 0].astype(np.float64), p1[:, 1].astype(np.float64)
    x2, y2 = p2[:, 0].astype(np.float64), p2[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        a = F[0] * x1 + F[1] * y1 + F[2]
        b = F[3] * x1 + F[4] * y1 + F[5]
        c = F[6] * x1 + F[7] * y1 + F[8]
        s2 = 1.0 / (a * a + b * b)
        d2 = x2 * a + y2 * b + c
        a = F[0] * x2 + F[3] * y2 + F[6]
        b = F[1] * x2 + F[4] * y2 + F[7]
        c = F[2] * x2 + F[5] * y2 + F[8]
        s1 = 1.0 / (a * a + b * b)
        d1 = x1 * a + y1 * b + c
        e1 = d1 * d1 * s1
        e2 = d2 * d2 * s2
        return np.where(e1 < e2, e2, e1).astype(np.float32)


def inliers(F, p1, p2, thresh):
    """findInliers: err <= (float)(thresh * thresh)"""
    return (errors(F, p1, p2) <= np.float32(thresh * thresh)).astype(np.uint8)


def median_bits(err):
    """nth_element over the f32 errors read as int32, position n/2 -> the int32 pattern"""
    v = np.sort(np.asarray(err, np.float32).view(np.int32))
    return int(v[len(v) // 2])


def bits_to_f32(b):
    return struct.unpack("<f", struct.pack("<i", int(b)))[0]


def sample_stream(p1, p2, n, path, max_iters, confidence, check=1, attempts=None):
    if path == "kernel":
        return [list(range(7))], 1
    ransac = path == "ransac"
    niters0 = max(max_iters, 1) if ransac else max(update_num_iters(confidence, LMEDS_OUTLIER_RATIO, MODEL_POINTS, max_iters), 3)
    niters0 = min(niters0, max_iters)
    rng = CvRng()
    subs = []
    while len(subs) < niters0:
        s = get_subset(rng, p1, p2, n, check, RANSAC_MAX_ATTEMPTS if ransac else LMEDS_MAX_ATTEMPTS, attempts)
        if s is None:
            break
        subs.append(s)
    return subs, niters0


def choose_path(n):
    return "kernel" if n == 7 else ("lmeds" if n < 15 else "ransac")


def walk(path, n, niters0, nsub, nmodels, score, confidence):
    """the sequential RANSAC / LMeDS walk over per-candidate scores -> (iters, best_iter, best_root, best_median)"""
    if path == "kernel":
        return 1, (0 if nmodels[0] > 0 else -1), (0 if nmodels[0] > 0 else -1), 0.0
    it, best_iter, best_root = 0, -1, -1
    niters = niters0
    if path == "ransac":
        max_good = 0
        while it < niters:
            if it >= nsub:
                break
            for m in range(int(nmodels[it])):
                good = int(score[it][m])
                if good > max(max_good, MODEL_POINTS - 1):
                    best_iter, best_root, max_good = it, m, good
                    niters = update_num_iters(confidence, (n - good) / n, MODEL_POINTS, niters)
            it += 1
        return it, best_iter, best_root, 0.0
    min_median = DBL_MAX
    while it < niters:
        if it >= nsub:
            break
        for m in range(int(nmodels[it])):
            med = bits_to_f32(score[it][m])
            if med < min_median:
                min_median, best_iter, best_root = med, it, m
        it += 1
    return it, best_iter, best_root, (min_median if best_iter >= 0 else 0.0)


def lmeds_sigma(n, min_median):
    sigma = 2.5 * 1.4826 * (1 + 5.0 / (n - MODEL_POINTS)) * math.sqrt(min_median)
    return max(sigma, 0.001)


def final_mask(path, n, F, best_iter, best_median, p1, p2, threshold):
    if path == "kernel":
        return np.ones(n, np.uint8)
    if best_iter < 0:
        return np.zeros(n, np.uint8)
    thr = lmeds_sigma(n, best_median) if path == "lmeds" else threshold
    return inliers(F, p1, p2, thr)


def lmeds_rounding_decided(path, n, dev_best, ref_best, dev_score, ref_score):
    """a status difference traced to LMeDS's choice at rounding level: for n <= 13 the n/2-th error of every candidate is
    one of the 7 it fits exactly, so the medians compared are rounding noise (~1e-26) and a last-bit difference of a
    candidate's F moves its median.  True when the two walks chose different candidates and at least one of the two
    winners has a different median on the device than in the restatement."""
    if path != "lmeds" or n // 2 >= MODEL_POINTS or tuple(dev_best) == tuple(ref_best) or min(dev_best[0], ref_best[0]) < 0:
        return False
    return any(int(dev_score[h][m]) != int(ref_score[h][m]) for h, m in (dev_best, ref_best))


def score_candidates(path, F, p1, p2, threshold):
    """a candidate's score as the device reports it: inlier count (RANSAC, kernel) or the median's int32 bits (LMeDS)"""
    e = errors(F, p1, p2)
    if path == "lmeds":
        return median_bits(e)
    return int(np.count_nonzero(e <= np.float32(threshold * threshold)))


def find(pts1, pts2, threshold=1.0, confidence=0.99, max_iters=1000, check=1):
    """findFundamentalMat -> (status [n] uint8, trace).  Only the hypotheses the walk reaches are solved and scored (the
    walk is replayed as it goes); the trace's subsets are the whole stream, as the device's are."""
    p1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
    n = len(p1)
    if n < 7:
        raise ValueError("n < 7")
    if threshold <= 0:
        threshold = 3.0
    if confidence < DBL_EPSILON or confidence > 1 - DBL_EPSILON:
        confidence = 0.99
    path = choose_path(n)
    subs, niters0 = sample_stream(p1, p2, n, path, max_iters, confidence, check)
    Fs, nm, sc = [], [], []
    # the walk, scoring each hypothesis as it is reached
    niters, it, best_iter, best_root, max_good, min_median = niters0, 0, -1, -1, 0, DBL_MAX
    limit = 1 if path == "kernel" else niters
    while it < limit and it < len(subs):
        idx = subs[it]
        cands = run7point(p1[idx], p2[idx])
        Fs.append(cands)
        nm.append(len(cands))
        sc.append([score_candidates(path, F, p1, p2, threshold) for F in cands])
        if path == "ransac":
            for m, good in enumerate(sc[-1]):
                if good > max(max_good, MODEL_POINTS - 1):
                    best_iter, best_root, max_good = it, m, good
                    niters = update_num_iters(confidence, (n - good) / n, MODEL_POINTS, niters)
            limit = niters
        elif path == "lmeds":
            for m, b in enumerate(sc[-1]):
                med = bits_to_f32(b)
                if med < min_median:
                    min_median, best_iter, best_root = med, it, m
        it += 1
    if path == "kernel":
        best_iter, best_root = (0, 0) if nm[0] > 0 else (-1, -1)
        it = 1
    best_median = min_median if (path == "lmeds" and best_iter >= 0) else 0.0
    F = np.array(Fs[best_iter][best_root] if best_iter >= 0 else [0.0] * 9, np.float64)
    status = final_mask(path, n, F, best_iter, best_median, p1, p2, threshold)
    F27 = np.zeros((len(Fs), 3, 9))
    for i, c in enumerate(Fs):
        for m, f in enumerate(c):
            F27[i, m] = f
    score = np.zeros((len(Fs), 3), np.int64)
    for i, s in enumerate(sc):
        score[i, :len(s)] = s
    trace = dict(path=path, subsets=np.array(subs, np.int32).reshape(-1, 7), n_subsets=len(subs), nmodels=np.array(nm, np.int32),
                 F=F27.reshape(-1, 3, 3, 3), score=score, iters=it, best_iter=best_iter, best_root=best_root, best_median=best_median,
                 F_best=F.reshape(3, 3), niters0=niters0, n_inliers=int(status.sum()))
    return status, trace


# ---------------------------------------------------------------------------------------------- synthetic two-view scenes
FOCAL_LENGTH = 460.0


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def true_F(R, t, col=752, row=480):
    """x2' F x1 = 0 for x2 = R x1 + t, pixels = FOCAL_LENGTH * x/z + (col/2, row/2)"""
    K = np.array([[FOCAL_LENGTH, 0, col / 2.0], [0, FOCAL_LENGTH, row / 2.0], [0, 0, 1]])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    return Ki.T @ tx @ R @ Ki


def two_view(n, outliers=0.0, noise=0.0, seed=0, kind="general", col=752, row=480):
    """un_cur, un_forw [n, 2] f32 in rejectWithF's pixel frame, the inlier truth [n] bool, and (R, t)"""
    rs = np.random.RandomState(seed)
    K = np.array([[FOCAL_LENGTH, 0, col / 2.0], [0, FOCAL_LENGTH, row / 2.0], [0, 0, 1]])
    R, t = rot(*rs.uniform(-0.05, 0.05, 3)), np.array([0.3, 0.05, 0.1]) * rs.uniform(0.5, 1.5)
    if kind == "rotation":
        t = np.zeros(3)
    if kind == "zero":
        R, t = np.eye(3), np.zeros(3)
    px = np.c_[rs.uniform(20, col - 20, n), rs.uniform(20, row - 20, n)]
    if kind == "collinear":
        u = rs.uniform(0, 1, n)
        px = np.c_[40 + u * (col - 80), 60 + u * (row - 120) + rs.normal(0, 1e-3, n)]
    if kind == "planar":
        ray = np.c_[(px - K[:2, 2]) / FOCAL_LENGTH, np.ones(n)]
        nrm, dist = np.array([0.1, -0.2, 1.0]), 5.0
        X = ray * (dist / (ray @ nrm))[:, None]
    else:
        X = np.c_[(px - K[:2, 2]) / FOCAL_LENGTH, np.ones(n)] * rs.uniform(2, 20, n)[:, None]
    if kind == "duplicates":
        k = max(1, n // 4)
        X[n - k:] = X[rs.randint(0, n - k, k)]
    X2 = X @ R.T + t
    p1 = (X @ K.T)[:, :2] / X[:, 2:3]
    p2 = (X2 @ K.T)[:, :2] / X2[:, 2:3]
    if noise > 0:
        p2 = p2 + rs.normal(0, noise, p2.shape)
    truth = np.ones(n, bool)
    k = int(round(outliers * n))
    if k:
        bad = rs.choice(n, k, replace=False)
        p2[bad] += rs.uniform(15, 60, (k, 2)) * rs.choice([-1, 1], (k, 2))
        truth[bad] = False
    return p1.astype(np.float32), p2.astype(np.float32), truth, (R, t)
