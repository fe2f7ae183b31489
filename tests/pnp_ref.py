"""Host restatement of include/lvi_pnp.h: OpenCV 4.5.x cv::solvePnPRansac(matched_3d, matched_2d_old_norm,
K = I, D = empty, rvec, t, true, 100, 10.0 / 460.0, 0.99, inliers) as KeyFrame::PnPRANSAC calls it (keyframe.cpp:163),
reduced to what findConnection reads afterwards: the inlier status.

Scalar Python floats (IEEE double, one rounding per operation, no fused multiply-add) in the operation order of
csrc/lvi_pnp_math.hpp; numpy only where every element sees the same scalar operations in the same order (the 12x12 Jacobi
rounds, M'M, the errors).  `solve` returns the status and a trace shaped like pnp.PnPRansac.trace() plus the walk's info.

Not restated: the P3P path of n == 4, the extrinsic guess (it does not enter an EPnP kernel), the final
SOLVEPNP_ITERATIVE refit (it changes the pose, never `inliers`), and the Rodrigues round trip of the model between the
kernel and the error (the errors are scored with EPnP's R directly)."""
import math

import numpy as np

from fmat_ref import CvRng, update_num_iters

MODEL_POINTS = 5
SWEEPS12 = 8                # round-robin Jacobi sweeps of the 12x12 problem (11 rounds of 6 pairs each); DESIGN §16
SWEEPS3 = 8                 # cyclic Jacobi sweeps of the 3x3 eigenproblem and of the one-sided 3x3 SVD
GN_STEPS = 5
NAN = float("nan")
THRESHOLD = float(np.float32(10.0 / 460.0))        # the `float reprojectionError` parameter
CONFIDENCE = 0.99
MAX_ITERS = 100


# ------------------------------------------------------------------------------------------------ C semantics
def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(x):
    return math.sqrt(x) if x >= 0 else (NAN if x == x else x)


# ------------------------------------------------------------------------------------------------ the sample stream
def get_subset(rng, n):
    """RANSACPointSetRegistrator::getSubset with modelPoints = 5: distinct indices, duplicates redrawn; the PnP callback
    has no checkSubset, so the first draw of five is the subset"""
    idx = []
    for _ in range(MODEL_POINTS):
        k = rng.uniform(0, n)
        while k in idx:
            k = rng.uniform(0, n)
        idx.append(k)
    return idx


def sample_stream(n, max_iters):
    if n == MODEL_POINTS:
        return [list(range(MODEL_POINTS))]
    rng = CvRng()
    return [get_subset(rng, n) for _ in range(max_iters)]


# ------------------------------------------------------------------------------------------------ decompositions
def _rot(apq, app, aqq):
    """the Jacobi rotation (c, s) that zeroes a_pq of a symmetric matrix"""
    if apq == 0.0:
        return 1.0, 0.0
    theta = _div(aqq - app, 2.0 * apq)
    t = _div(-1.0 if theta < 0 else 1.0, abs(theta) + _sqrt(theta * theta + 1.0))
    c = _div(1.0, _sqrt(t * t + 1.0))
    return c, t * c


def eig3_jacobi(S):
    """symmetric 3x3: SWEEPS3 cyclic sweeps over (0,1) (0,2) (1,2), rows then columns -> (lam [3] descending, ties to the
    lower index; E [3][3] with the eigenvectors in its columns, same order)"""
    a = [list(map(float, r)) for r in S]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS3):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            c, s = _rot(a[p][q], a[p][p], a[q][q])
            for j in range(3):
                x, y = a[p][j], a[q][j]
                a[p][j], a[q][j] = c * x - s * y, s * x + c * y
            for i in range(3):
                x, y = a[i][p], a[i][q]
                a[i][p], a[i][q] = c * x - s * y, s * x + c * y
            for i in range(3):
                x, y = v[i][p], v[i][q]
                v[i][p], v[i][q] = c * x - s * y, s * x + c * y
    lam = [a[0][0], a[1][1], a[2][2]]
    order, used = [], [False] * 3
    for _ in range(3):
        best = -1
        for i in range(3):
            if used[i]:
                continue
            if best < 0 or lam[i] > lam[best]:
                best = i
        used[best] = True
        order.append(best)
    return [lam[i] for i in order], [[v[r][i] for i in order] for r in range(3)]


def round_pairs(r):
    """round r (0..10) of the round-robin schedule on 12 indices: six disjoint pairs (p < q)"""
    out = [(r, 11)]
    for k in range(1, 6):
        a, b = (r + k) % 11, (r - k + 11) % 11
        out.append((min(a, b), max(a, b)))
    return out


_ROUNDS = []
for _r in range(11):
    _pairs = round_pairs(_r)
    _P = np.array([p for p, _ in _pairs])
    _Q = np.array([q for _, q in _pairs])
    _partner = np.zeros(12, np.int64)
    _pair_of = np.zeros(12, np.int64)
    _is_p = np.zeros(12, bool)
    for _k, (_p, _q) in enumerate(_pairs):
        _partner[_p], _partner[_q] = _q, _p
        _pair_of[_p] = _pair_of[_q] = _k
        _is_p[_p] = True
    _ROUNDS.append((_P, _Q, _partner, _pair_of, _is_p))


def eig12_jacobi(S, sweeps=SWEEPS12, residue=False):
    """symmetric 12x12 by round-robin Jacobi: per round all six (c, s) from the current matrix, then the row rotations,
    then the column rotations (of the matrix and of V); a fixed number of sweeps -> (lam [12] = the diagonal, V [12][12])"""
    A = np.array(S, np.float64)
    V = np.eye(12)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for P, Q, partner, pair_of, is_p in _ROUNDS:
                apq, app, aqq = A[P, Q], A[P, P], A[Q, Q]
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta < 0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                zero = apq == 0.0
                c = np.where(zero, 1.0, c)
                s = np.where(zero, 0.0, s)
                ca = c[pair_of]
                cb = np.where(is_p, -s[pair_of], s[pair_of])
                A = ca[:, None] * A + cb[:, None] * A[partner, :]         # p: c a_p - s a_q;  q: s a_p + c a_q
                A = A * ca[None, :] + A[:, partner] * cb[None, :]
                V = V * ca[None, :] + V[:, partner] * cb[None, :]
    lam = np.diag(A).copy()
    if residue:
        off = A - np.diag(lam)
        return lam, V, float(np.sqrt((off * off).sum()) / max(np.abs(lam).max(), 1e-300))
    return lam, V


def smallest4(lam):
    """indices of v[0..3]: the eigenvectors of the four smallest eigenvalues, v[0] the smallest; of a descending sort
    whose ties go to the lower index these are the last four, so among equals the higher index comes first here"""
    out, used = [], [False] * 12
    for _ in range(4):
        best = -1
        for i in range(12):
            if used[i]:
                continue
            if best < 0 or lam[i] <= lam[best]:
                best = i
        used[best] = True
        out.append(best)
    return out


def inv3(M):
    """Gauss-Jordan with partial pivoting (first largest |pivot|) on [M | I]; None on an exactly zero pivot"""
    a = [list(map(float, M[i])) + [1.0 if j == i else 0.0 for j in range(3)] for i in range(3)]
    for c in range(3):
        p, best = c, abs(a[c][c])
        for i in range(c + 1, 3):
            if abs(a[i][c]) > best:
                best, p = abs(a[i][c]), i
        if best == 0:
            return None
        if p != c:
            a[c], a[p] = a[p], a[c]
        d = a[c][c]
        for j in range(6):
            a[c][j] = _div(a[c][j], d)
        for i in range(3):
            if i == c:
                continue
            f = a[i][c]
            for j in range(6):
                a[i][j] = a[i][j] - f * a[c][j]
    return [row[3:] for row in a]


def lstsq(A, b):
    """min |A x - b| for a small dense A [nr][nc], nr >= nc: Householder QR column by column (each column scaled by its
    largest |entry| first), Q'b, back substitution.  A column that is exactly zero below the diagonal: x = 0."""
    nr, nc = len(A), len(A[0])
    a = [list(map(float, r)) for r in A]
    b = list(map(float, b))
    a1, a2 = [0.0] * nc, [0.0] * nc
    for k in range(nc):
        eta = 0.0
        for i in range(k, nr):
            e = abs(a[i][k])
            if eta < e:
                eta = e
        if eta == 0:
            return [0.0] * nc
        inv_eta = _div(1.0, eta)
        sum2 = 0.0
        for i in range(k, nr):
            a[i][k] = a[i][k] * inv_eta
            sum2 = sum2 + a[i][k] * a[i][k]
        sigma = _sqrt(sum2)
        if a[k][k] < 0:
            sigma = -sigma
        a[k][k] = a[k][k] + sigma
        a1[k] = sigma * a[k][k]
        a2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s = 0.0
            for i in range(k, nr):
                s = s + a[i][k] * a[i][j]
            tau = _div(s, a1[k])
            for i in range(k, nr):
                a[i][j] = a[i][j] - tau * a[i][k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau = tau + a[i][j] * b[i]
        tau = _div(tau, a1[j])
        for i in range(j, nr):
            b[i] = b[i] - tau * a[i][j]
    x = [0.0] * nc
    for i in range(nc - 1, -1, -1):
        s = 0.0
        for j in range(i + 1, nc):
            s = s + a[i][j] * x[j]
        x[i] = _div(b[i] - s, a2[i])
    return x


def polar3_jacobi(B):
    """R = U V' of the SVD of B (3x3) by one-sided Jacobi: SWEEPS3 cyclic sweeps over the column pairs (0,1) (0,2) (1,2),
    then U's columns are B's divided by their norms"""
    b = [list(map(float, r)) for r in B]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS3):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            al = b[0][p] * b[0][p] + b[1][p] * b[1][p] + b[2][p] * b[2][p]
            be = b[0][q] * b[0][q] + b[1][q] * b[1][q] + b[2][q] * b[2][q]
            ga = b[0][p] * b[0][q] + b[1][p] * b[1][q] + b[2][p] * b[2][q]
            c, s = _rot(ga, al, be)
            for i in range(3):
                x, y = b[i][p], b[i][q]
                b[i][p], b[i][q] = c * x - s * y, s * x + c * y
            for i in range(3):
                x, y = v[i][p], v[i][q]
                v[i][p], v[i][q] = c * x - s * y, s * x + c * y
    for j in range(3):
        nrm = _sqrt(b[0][j] * b[0][j] + b[1][j] * b[1][j] + b[2][j] * b[2][j])
        for i in range(3):
            b[i][j] = _div(b[i][j], nrm)
    return [[b[i][0] * v[k][0] + b[i][1] * v[k][1] + b[i][2] * v[k][2] for k in range(3)] for i in range(3)]


# ------------------------------------------------------------------------------------------------ EPnP
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
BETA_COLS = {1: (0, 1, 3, 6), 2: (0, 1, 2), 3: (0, 1, 2, 3, 4)}


def control_points(pw, eig):
    n = len(pw)
    c0 = [0.0, 0.0, 0.0]
    for p in pw:
        for j in range(3):
            c0[j] = c0[j] + p[j]
    for j in range(3):
        c0[j] = _div(c0[j], float(n))
    S = [[0.0] * 3 for _ in range(3)]
    for p in pw:
        d = [p[0] - c0[0], p[1] - c0[1], p[2] - c0[2]]
        for i in range(3):
            for j in range(i, 3):
                S[i][j] = S[i][j] + d[i] * d[j]
    for i in range(3):
        for j in range(i):
            S[i][j] = S[j][i]
    if eig == "lapack":
        w, E = np.linalg.eigh(np.array(S))
        lam = [float(w[2 - k]) for k in range(3)]
        E = [[float(E[r][2 - k]) for k in range(3)] for r in range(3)]
    else:
        lam, E = eig3_jacobi(S)
    cws = [c0]
    for k in range(3):
        # the axis's sign: its largest |component| (the first of equals) is made positive.  With noisy image points EPnP's
        # answer depends on the signs of the control axes, so they cannot be left to the decomposition
        big = 0
        for j in range(1, 3):
            if abs(E[j][k]) > abs(E[big][k]):
                big = j
        if E[big][k] < 0:
            for j in range(3):
                E[j][k] = -E[j][k]
        f = _sqrt(_div(lam[k], float(n)))
        cws.append([c0[j] + f * E[j][k] for j in range(3)])
    return cws


def barycentric(pw, cws):
    c0 = cws[0]
    CC = [[cws[j + 1][i] - c0[i] for j in range(3)] for i in range(3)]
    ci = inv3(CC)
    if ci is None:
        return None
    al = []
    for p in pw:
        d = [p[0] - c0[0], p[1] - c0[1], p[2] - c0[2]]
        a = [0.0] * 4
        for j in range(3):
            a[1 + j] = ci[j][0] * d[0] + ci[j][1] * d[1] + ci[j][2] * d[2]
        a[0] = 1.0 - a[1] - a[2] - a[3]
        al.append(a)
    return al


def fill_m(al, uv):
    M = np.zeros((2 * len(al), 12))
    for i, (a, (u, v)) in enumerate(zip(al, uv)):
        for j in range(4):
            M[2 * i, 3 * j] = a[j]
            M[2 * i, 3 * j + 2] = -(a[j] * u)
            M[2 * i + 1, 3 * j + 1] = a[j]
            M[2 * i + 1, 3 * j + 2] = -(a[j] * v)
    return M


def mtm(M):
    S = np.zeros((12, 12))
    for r in range(len(M)):
        S = S + M[r][:, None] * M[r][None, :]
    return S


def l_and_rho(v4, cws):
    """L (6x10) from the four null vectors v4 [4][12], rho [6] from the control points"""
    L, rho = [], []
    for a, b in PAIRS:
        dv = [[v4[k][3 * a + j] - v4[k][3 * b + j] for j in range(3)] for k in range(4)]

        def dot(x, y):
            return dv[x][0] * dv[y][0] + dv[x][1] * dv[y][1] + dv[x][2] * dv[y][2]
        L.append([dot(0, 0), 2.0 * dot(0, 1), dot(1, 1), 2.0 * dot(0, 2), 2.0 * dot(1, 2), dot(2, 2), 2.0 * dot(0, 3), 2.0 * dot(1, 3), 2.0 * dot(2, 3),
                  dot(3, 3)])
        d = [cws[a][j] - cws[b][j] for j in range(3)]
        rho.append(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return L, rho


def beta_init(N, L, rho):
    cols = BETA_COLS[N]
    b = lstsq([[row[c] for c in cols] for row in L], rho)
    if N == 1:
        if b[0] < 0:
            b0 = _sqrt(-b[0])
            return [b0, _div(-b[1], b0), _div(-b[2], b0), _div(-b[3], b0)]
        b0 = _sqrt(b[0])
        return [b0, _div(b[1], b0), _div(b[2], b0), _div(b[3], b0)]
    if b[0] < 0:
        b0 = _sqrt(-b[0])
        b1 = _sqrt(-b[2]) if b[2] < 0 else 0.0
    else:
        b0 = _sqrt(b[0])
        b1 = _sqrt(b[2]) if b[2] > 0 else 0.0
    if b[1] < 0:
        b0 = -b0
    return [b0, b1, 0.0, 0.0] if N == 2 else [b0, b1, _div(b[3], b0), 0.0]


def gauss_newton(L, rho, be):
    be = list(be)
    for _ in range(GN_STEPS):
        A, r = [], []
        for i in range(6):
            l = L[i]
            A.append([2.0 * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3],
                      l[1] * be[0] + 2.0 * l[2] * be[1] + l[4] * be[2] + l[7] * be[3],
                      l[3] * be[0] + l[4] * be[1] + 2.0 * l[5] * be[2] + l[8] * be[3],
                      l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2.0 * l[9] * be[3]])
            r.append(rho[i] - (l[0] * be[0] * be[0] + l[1] * be[0] * be[1] + l[2] * be[1] * be[1] + l[3] * be[0] * be[2] + l[4] * be[1] * be[2] +
                              l[5] * be[2] * be[2] + l[6] * be[0] * be[3] + l[7] * be[1] * be[3] + l[8] * be[2] * be[3] + l[9] * be[3] * be[3]))
        x = lstsq(A, r)
        be = [be[k] + x[k] for k in range(4)]
    return be


def pose_from_betas(be, v4, al, pw, uv, eig):
    """compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error -> (R [3][3], t [3], rep)"""
    n = len(pw)
    ccs = [[0.0] * 3 for _ in range(4)]
    for k in range(4):
        for j in range(4):
            for c in range(3):
                ccs[j][c] = ccs[j][c] + be[k] * v4[k][3 * j + c]
    pcs = [[a[0] * ccs[0][c] + a[1] * ccs[1][c] + a[2] * ccs[2][c] + a[3] * ccs[3][c] for c in range(3)] for a in al]
    if pcs[0][2] < 0:
        pcs = [[-x for x in p] for p in pcs]             # (the ccs are not read again)
    pc0, pw0 = [0.0] * 3, [0.0] * 3
    for i in range(n):
        for j in range(3):
            pc0[j] = pc0[j] + pcs[i][j]
            pw0[j] = pw0[j] + pw[i][j]
    for j in range(3):
        pc0[j] = _div(pc0[j], float(n))
        pw0[j] = _div(pw0[j], float(n))
    AB = [[0.0] * 3 for _ in range(3)]
    for i in range(n):
        for j in range(3):
            for k in range(3):
                AB[j][k] = AB[j][k] + (pcs[i][j] - pc0[j]) * (pw[i][k] - pw0[k])
    if eig == "lapack":
        with np.errstate(all="ignore"):
            try:
                U, _, Vt = np.linalg.svd(np.array(AB))
                R = [[float(x) for x in row] for row in U @ Vt]
            except (np.linalg.LinAlgError, ValueError):
                R = [[NAN] * 3 for _ in range(3)]
    else:
        R = polar3_jacobi(AB)
    det = (R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] - R[0][2] * R[1][1] * R[2][0] -
           R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1])
    if det < 0:
        R[2] = [-x for x in R[2]]
    t = [pc0[i] - (R[i][0] * pw0[0] + R[i][1] * pw0[1] + R[i][2] * pw0[2]) for i in range(3)]
    s = 0.0
    for i in range(n):
        p = pw[i]
        xc = R[0][0] * p[0] + R[0][1] * p[1] + R[0][2] * p[2] + t[0]
        yc = R[1][0] * p[0] + R[1][1] * p[1] + R[1][2] * p[2] + t[1]
        iz = _div(1.0, R[2][0] * p[0] + R[2][1] * p[1] + R[2][2] * p[2] + t[2])
        du, dv = uv[i][0] - xc * iz, uv[i][1] - yc * iz
        s = s + _sqrt(du * du + dv * dv)
    return R, t, _div(s, float(n))


def epnp(pts3d, pts2d, eig="jacobi", detail=False):
    """epnp::compute_pose on the given points (f32 inputs, everything in double, fu = fv = 1, uc = vc = 0) ->
    None (no model: an exactly singular control-point matrix) or dict(R, t, which_beta, rep)"""
    pw = [[float(v) for v in p] for p in np.asarray(pts3d, np.float32).reshape(-1, 3)]
    uv = [[float(v) for v in p] for p in np.asarray(pts2d, np.float32).reshape(-1, 2)]
    cws = control_points(pw, eig)
    al = barycentric(pw, cws)
    if al is None:
        return None
    S = mtm(fill_m(al, uv))
    if eig == "lapack":
        with np.errstate(all="ignore"):
            try:
                lam, V = np.linalg.eigh(S)
            except (np.linalg.LinAlgError, ValueError):
                lam, V = np.full(12, NAN), np.full((12, 12), NAN)
        idx = [0, 1, 2, 3]
    else:
        lam, V = eig12_jacobi(S)
        idx = smallest4([float(x) for x in lam])
    v4 = [[float(V[r][i]) for r in range(12)] for i in idx]
    L, rho = l_and_rho(v4, cws)
    cand = {}
    for N in (1, 2, 3):
        be = gauss_newton(L, rho, beta_init(N, L, rho))
        cand[N] = pose_from_betas(be, v4, al, pw, uv, eig) + (be,)
    N = 1
    if cand[2][2] < cand[1][2]:
        N = 2
    if cand[3][2] < cand[N][2]:
        N = 3
    out = dict(R=np.array(cand[N][0]), t=np.array(cand[N][1]), which_beta=N, rep=cand[N][2])
    if detail:
        out.update(S=S, lam=np.array(lam), V=np.array(V), v4=np.array(v4), cand=cand, L=L, rho=rho, alphas=al, cws=cws)
    return out


# ------------------------------------------------------------------------------------------------ error, walk, solve
def errors(R, t, pts3d, pts2d):
    """PnPRansacCallback::computeError -> projectPoints with K = I and no distortion: f32 errors"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    p = np.asarray(pts3d, np.float32).reshape(-1, 3).astype(np.float64)
    q = np.asarray(pts2d, np.float32).reshape(-1, 2)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        X = R[0, 0] * x + R[0, 1] * y + R[0, 2] * z + t[0]
        Y = R[1, 0] * x + R[1, 1] * y + R[1, 2] * z + t[1]
        Z = R[2, 0] * x + R[2, 1] * y + R[2, 2] * z + t[2]
        iz = np.where(Z != 0, 1.0 / Z, 1.0)
        u = (X * iz).astype(np.float32)
        v = (Y * iz).astype(np.float32)
        dx, dy = q[:, 0] - u, q[:, 1] - v
        return dx * dx + dy * dy                                          # f32 throughout


def threshold_f32(threshold):
    """the callback's `float t = (float)(threshold * threshold)` on the float parameter"""
    thr = float(np.float32(threshold))
    return np.float32(thr * thr)


def inliers(R, t, pts3d, pts2d, threshold):
    with np.errstate(all="ignore"):
        return (errors(R, t, pts3d, pts2d) <= threshold_f32(threshold)).astype(np.uint8)


def walk(n, max_iters, has_model, good, confidence=CONFIDENCE, nsub=None):
    """RANSACPointSetRegistrator::run over per-hypothesis (has_model, good) -> (iters, best_iter)"""
    nsub = len(good) if nsub is None else nsub
    if n == MODEL_POINTS:
        return 1, (0 if has_model[0] else -1)
    it, best, max_good, niters = 0, -1, 0, max_iters
    while it < niters and it < nsub:
        if has_model[it]:
            g = int(good[it])
            if g > max(max_good, MODEL_POINTS - 1):
                best, max_good = it, g
                niters = update_num_iters(confidence, (n - g) / n, MODEL_POINTS, niters)
        it += 1
    return it, best


_CACHE = {}


def solve(pts3d, pts2d, threshold=THRESHOLD, confidence=CONFIDENCE, max_iters=MAX_ITERS, eig="jacobi"):
    """solvePnPRansac's inliers -> (status [n] uint8, trace).  Only the hypotheses the walk reaches are solved."""
    p3 = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
    p2 = np.ascontiguousarray(pts2d, np.float32).reshape(-1, 2)
    n = len(p3)
    if n < MODEL_POINTS or len(p2) != n:
        raise ValueError("n < 5")
    key = (p3.tobytes(), p2.tobytes(), float(threshold), float(confidence), int(max_iters), eig)
    if key in _CACHE:
        st, T = _CACHE[key]
        return st.copy(), T
    direct = n == MODEL_POINTS
    subs = sample_stream(n, max_iters)
    models, has, good = [], [], []
    it, best, max_good, niters = 0, -1, 0, (1 if direct else max_iters)
    while it < niters and it < len(subs):
        m = epnp(p3[subs[it]], p2[subs[it]], eig)
        models.append(m)
        has.append(m is not None)
        g = int(inliers(m["R"], m["t"], p3, p2, threshold).sum()) if m is not None else 0
        good.append(g)
        if direct:
            best = 0 if m is not None else -1
        elif m is not None and g > max(max_good, MODEL_POINTS - 1):
            best, max_good = it, g
            niters = update_num_iters(confidence, (n - g) / n, MODEL_POINTS, niters)
        it += 1
    if best < 0:
        status = np.zeros(n, np.uint8)
    elif direct:
        status = np.ones(n, np.uint8)
    else:
        status = inliers(models[best]["R"], models[best]["t"], p3, p2, threshold)
    T = dict(path="direct" if direct else "ransac", subsets=np.array(subs, np.int32).reshape(-1, MODEL_POINTS), n_subsets=len(subs), iters=it,
             best_iter=best, n_inliers=int(status.sum()), has_model=np.array(has, bool), good=np.array(good, np.int64), models=models,
             R=models[best]["R"] if best >= 0 else np.zeros((3, 3)), t=models[best]["t"] if best >= 0 else np.zeros(3),
             which_beta=models[best]["which_beta"] if best >= 0 else 0)
    _CACHE[key] = (status.copy(), T)
    return status, T


# ------------------------------------------------------------------------------------------------ scenes
FOCAL_LENGTH = 460.0


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = float(np.linalg.norm(r))
    if th == 0:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def scene(n, outliers=0.0, noise=0.0, seed=0, kind="general"):
    """matched_3d [n, 3], matched_2d_old_norm [n, 2] (f32), the inlier truth [n] and (R, t): 3D points uniform in
    [-4,4] x [-3,3] x [4,12], rotation of axis-angle 0.2 N(0,1)^3, translation 0.5 N(0,1)^3, uv = (X/Z, Y/Z) + N(0, noise),
    floor(outliers n) points replaced by uniform uv in +-0.8.  kind: "planar" (z = 8 exactly), "identical" (one point)."""
    rs = np.random.RandomState(seed)
    P = np.c_[rs.uniform(-4, 4, n), rs.uniform(-3, 3, n), rs.uniform(4, 12, n)]
    if kind == "planar":
        P[:, 2] = 8.0
    if kind == "identical":
        P[:] = P[0]
    R, t = rodrigues(0.2 * rs.normal(0, 1, 3)), 0.5 * rs.normal(0, 1, 3)
    P = P.astype(np.float32)
    C = P.astype(np.float64) @ R.T + t
    uv = C[:, :2] / C[:, 2:3]
    if noise > 0:
        uv = uv + rs.normal(0, noise, uv.shape)
    truth = np.ones(n, bool)
    k = int(math.floor(outliers * n))
    if k:
        bad = rs.choice(n, k, replace=False)
        uv[bad] = rs.uniform(-0.8, 0.8, (k, 2))
        truth[bad] = False
    return P, uv.astype(np.float32), truth, (R, t)


# the GPU tier's calls (tests/test_gpu_pnp.py); tests/test_pnp_ref.py asserts on the restatement alone that none of them
# is rounding-decided (identical status, inlier count and iteration count under eig="jacobi" and eig="lapack")
GPU_NS = (5, 6, 26, 63, 64, 65, 150, 2048)
GPU_OUTLIERS = (0.0, 0.2, 0.4)
GPU_NOISE = (0.0, 0.5 / FOCAL_LENGTH, 2.0 / FOCAL_LENGTH)
GPU_SEEDS = (0, 1)
# cells removed when the list was written because they failed that condition: (n, outliers, noise index, seed)
GPU_REMOVED = ((63, 0.2, 2, 1), (150, 0.4, 2, 0))


def gpu_cases():
    out = []
    for n in GPU_NS:
        for o in GPU_OUTLIERS:
            if o > 0 and int(math.floor(o * n)) == 0:
                continue                                                   # no outlier results: the cell repeats the o = 0 one
            for ni, noise in enumerate(GPU_NOISE):
                for s in GPU_SEEDS:
                    if (n, o, ni, s) in GPU_REMOVED:
                        continue
                    out.append((n, o, noise, 1000 * n + 100 * ni + 10 * int(round(10 * o)) + s))
    return out


# Exact geometry (noise 0, inputs rounded to f32): the largest reprojection error and pose error against the scene's truth
# that epnp(eig="lapack") leaves, measured over scene(5, seed) and scene(50, seed) for seeds 0..19 and over the chosen
# hypothesis of every noise-0 call of gpu_cases() whose subset holds true inliers only (42 calls).  Measured on the LAPACK
# variant, not on the code under test; the tests assert 10 times these.
EXACT_REP, EXACT_DR, EXACT_DT = 1.8e-8, 1.1e-7, 1.1e-6
