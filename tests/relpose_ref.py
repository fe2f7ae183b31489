"""Reference of the initial two-view pose (include/lvi_relpose.h): a restatement of OpenCV 4.5.x
cv::recoverPose / decomposeEssentialMat (calib3d/src/five-point.cpp) and triangulatePoints (triangulate.cpp) as
MotionEstimator::solveRelativeRT (solve_5pts.cpp:193-227) calls them, and of Estimator::relativePose (estimator.cpp:493-522),
in plain Python float64.  Every sum is written out term by term, left to right: csrc/lvi_relpose_math.hpp and the device
must give these bits.  The SVD of E is the restatement's own (one-sided Jacobi on E'); the same pipeline is given a second
time over numpy.linalg.svd and a third time in mpmath at 50 digits.  Seeded scene generators are at the end.  Nothing here
reads the library."""
import math

import mpmath as mp
import numpy as np

import fmat_ref
from fman_ref import mul33

WINDOW = 10
MAX_SWEEPS = 30
SVD_EPS = 2.0 ** -52
DBL_MAX = 1.7976931348623157e308
FLAG_DEGENERATE, FLAG_NO_MODEL, FLAG_TOO_FEW = 1, 2, 4
DIST, THRESHOLD, CONFIDENCE = 50.0, 0.3 / 460, 0.99
MIN_PAIRS_SOLVE, MIN_INLIERS, MIN_PAIRS_GATE, FOCAL, MIN_PARALLAX_PX = 15, 12, 20, 460, 30
MP_DIGITS = 50
NAN = float("nan")


def _div(a, b):
    """IEEE division of two floats"""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _rotation(zeta_num_a, zeta_num_b, gamma):
    zeta = (zeta_num_b - zeta_num_a) / (2.0 * gamma)
    root = math.sqrt(1.0 + zeta * zeta)
    t = -1.0 / (-zeta + root) if zeta < 0 else 1.0 / (zeta + root)
    c = 1.0 / math.sqrt(1.0 + t * t)
    return c, c * t


def svd_null_vector(A):
    """lvi_fman_math::svd_null_vector on a list of rows of 4 floats (overwritten) -> (v [4], sweeps)"""
    rows = len(A)
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    sweeps = 0
    while sweeps < MAX_SWEEPS:
        sweeps += 1
        rotated = 0
        for p in range(3):
            for q in range(p + 1, 4):
                alpha = beta = gamma = 0.0
                for r in range(rows):
                    alpha = alpha + A[r][p] * A[r][p]
                    beta = beta + A[r][q] * A[r][q]
                    gamma = gamma + A[r][p] * A[r][q]
                if not abs(gamma) > SVD_EPS * math.sqrt(alpha * beta):
                    continue
                rotated += 1
                c, s = _rotation(alpha, beta, gamma)
                for M in (A, V):
                    for row in M:
                        mp_, mq = row[p], row[q]
                        row[p] = c * mp_ - s * mq
                        row[q] = s * mp_ + c * mq
        if rotated == 0:
            break
    best, least = 0, 0.0
    for c in range(4):
        n2 = 0.0
        for r in range(rows):
            n2 = n2 + A[r][c] * A[r][c]
        if c == 0 or n2 <= least:
            least, best = n2, c
    return [V[r][best] for r in range(4)], sweeps


def det33(A):
    return (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0])) + \
        A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0])


def _identity_pose():
    eye = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    return dict(R1=eye, R2=[r[:] for r in eye], t=[0.0] * 3, sv=[0.0] * 3, degenerate=1, sweeps=0)


def _finite(x):
    return abs(x) <= DBL_MAX


def _from_usv(U, Vt):
    """R1 = U W Vt, R2 = U W' Vt, t = U.col(2) after the two determinant rules"""
    if det33(U) < 0:
        U = [[-v for v in r] for r in U]
    if det33(Vt) < 0:
        Vt = [[-v for v in r] for r in Vt]
    UW = [[-U[r][1], U[r][0], U[r][2]] for r in range(3)]
    UWt = [[U[r][1], -U[r][0], U[r][2]] for r in range(3)]
    return mul33(UW, Vt), mul33(UWt, Vt), [U[r][2] for r in range(3)]


def decompose(E):
    """decomposeEssentialMat with the restatement's own SVD -> dict(R1, R2, t, sv, degenerate, sweeps)"""
    E = [[float(E[i][j]) for j in range(3)] for i in range(3)]
    D = _identity_pose()
    if not all(_finite(v) for r in E for v in r):
        return D
    B = [[E[c][r] for c in range(3)] for r in range(3)]
    J = [[1.0 if r == c else 0.0 for c in range(3)] for r in range(3)]
    sweeps = 0
    while sweeps < MAX_SWEEPS:
        sweeps += 1
        rotated = 0
        for p in range(2):
            for q in range(p + 1, 3):
                alpha = beta = gamma = 0.0
                for r in range(3):
                    alpha = alpha + B[r][p] * B[r][p]
                    beta = beta + B[r][q] * B[r][q]
                    gamma = gamma + B[r][p] * B[r][q]
                if not abs(gamma) > SVD_EPS * math.sqrt(alpha * beta):
                    continue
                rotated += 1
                c, s = _rotation(alpha, beta, gamma)
                for M in (B, J):
                    for row in M:
                        mp_, mq = row[p], row[q]
                        row[p] = c * mp_ - s * mq
                        row[q] = s * mp_ + c * mq
        if rotated == 0:
            break
    D["sweeps"] = sweeps
    w = [[(E[0][i] * J[0][k] + E[1][i] * J[1][k]) + E[2][i] * J[2][k] for i in range(3)] for k in range(3)]
    sig = [math.sqrt((w[k][0] * w[k][0] + w[k][1] * w[k][1]) + w[k][2] * w[k][2]) for k in range(3)]
    order = [0, 1, 2]
    for i in range(1, 3):
        j = i
        while j > 0 and sig[order[j]] > sig[order[j - 1]]:
            order[j], order[j - 1] = order[j - 1], order[j]
            j -= 1
    s0, s1, s2 = (sig[k] for k in order)
    if not s0 <= DBL_MAX or not s1 > 0.0:
        return D
    U = [[J[r][order[k]] for k in range(3)] for r in range(3)]
    v1, v2 = [w[order[0]][i] / s0 for i in range(3)], [w[order[1]][i] / s1 for i in range(3)]
    v3 = [v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]]
    R1, R2, t = _from_usv(U, [v1, v2, v3])
    return dict(R1=R1, R2=R2, t=t, sv=[s0, s1, s2], degenerate=0, sweeps=sweeps)


def decompose_numpy(E):
    """the same through numpy.linalg.svd: the independent route"""
    E = np.asarray(E, np.float64).reshape(3, 3)
    if not np.all(np.isfinite(E)):
        return _identity_pose()
    U, S, Vt = np.linalg.svd(E)
    if not S[1] > 0:
        return _identity_pose()
    R1, R2, t = _from_usv(U.tolist(), Vt.tolist())
    return dict(R1=R1, R2=R2, t=t, sv=S.tolist(), degenerate=0, sweeps=0)


def candidate(D, c):
    """[R1|t], [R2|t], [R1|-t], [R2|-t] -> 3 rows of 4"""
    R = D["R2"] if c & 1 else D["R1"]
    return [[R[r][0], R[r][1], R[r][2], -D["t"][r] if c >= 2 else D["t"][r]] for r in range(3)]


P0 = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]


def triangulation_matrix(P, x1, y1, x2, y2):
    return [[x1 * P0[2][k] - P0[0][k] for k in range(4)], [y1 * P0[2][k] - P0[1][k] for k in range(4)],
            [x2 * P[2][k] - P[0][k] for k in range(4)], [y2 * P[2][k] - P[1][k] for k in range(4)]]


def masks_of(P, Q, dist):
    """the four comparisons of recoverPose on one null vector -> (bit, the compared quantities)"""
    m = Q[2] * Q[3] > 0
    X, Y, Z, W = _div(Q[0], Q[3]), _div(Q[1], Q[3]), _div(Q[2], Q[3]), _div(Q[3], Q[3])
    m = m and Z < dist
    z2 = ((P[2][0] * X + P[2][1] * Y) + P[2][2] * Z) + P[2][3] * W
    m = m and z2 > 0
    m = m and z2 < dist
    return (1 if m else 0), (Q[2] * Q[3], Z, z2)


def cheirality(P, x1, y1, x2, y2, dist):
    Q, _ = svd_null_vector(triangulation_matrix(P, x1, y1, x2, y2))
    return masks_of(P, Q, dist)[0]


def choose(good):
    for c in range(4):
        if all(good[c] >= g for g in good):
            return c
    return 3


def _points(p):
    """cv::Point2f: float32, widened again"""
    return np.ascontiguousarray(p, np.float32).reshape(-1, 2).astype(np.float64).tolist()


def recover(E, pts1, pts2, mask=None, dist=DIST, route="own"):
    """cv::recoverPose with the identity camera matrix -> dict(R [3][3], t [3], good [4], chosen, n_inliers, flags, sv [3],
    cand [4] of (R, t), masks [4, n] uint8, mask [n] uint8).  route "numpy": the decomposition and every null vector by
    numpy.linalg.svd, and `margin`, the smallest relative distance of a compared quantity of an unmasked point from its
    threshold."""
    p1, p2 = _points(pts1), _points(pts2)
    n = len(p1)
    inm = np.ones(n, np.uint8) if mask is None else (np.asarray(mask).reshape(-1) != 0).astype(np.uint8)
    D = decompose(np.asarray(E, np.float64).reshape(3, 3).tolist()) if route == "own" else decompose_numpy(E)
    masks = np.zeros((4, n), np.uint8)
    cand = [(D["R2"] if c & 1 else D["R1"], [-v if c >= 2 else v for v in D["t"]]) for c in range(4)]
    margin = math.inf
    if not D["degenerate"]:
        for c in range(4):
            P = candidate(D, c)
            for k in range(n):
                if route == "own":
                    masks[c, k] = cheirality(P, p1[k][0], p1[k][1], p2[k][0], p2[k][1], dist) & inm[k]
                else:
                    A = np.array(triangulation_matrix(P, p1[k][0], p1[k][1], p2[k][0], p2[k][1]))
                    Q = np.linalg.svd(A)[2][3].tolist()
                    bit, (qq, Z, z2) = masks_of(P, Q, dist)
                    masks[c, k] = bit & inm[k]
                    if inm[k]:
                        near = [abs(qq), abs(Z - dist) / dist, abs(z2), abs(z2 - dist) / dist]
                        margin = min(margin, min(v for v in near if v == v))
    good = [int(masks[c].sum()) for c in range(4)]
    chosen = choose(good)
    return dict(R=cand[chosen][0], t=cand[chosen][1], good=good, chosen=chosen, n_inliers=good[chosen], flags=FLAG_DEGENERATE if D["degenerate"] else 0,
                sv=D["sv"], cand=cand, masks=masks, mask=masks[chosen].copy(), margin=margin, sweeps=D["sweeps"])


def with_mask(r, mask):
    """the result of recover(..., mask) from the result r of recover(..., None) on the same scene: the input mask is ANDed
    in after everything else, so the four raw masks are computed once and shared"""
    inm = (np.asarray(mask).reshape(-1) != 0).astype(np.uint8)
    masks = r["masks"] & inm[None, :]
    good = [int(m.sum()) for m in masks]
    chosen = choose(good)
    return dict(r, R=r["cand"][chosen][0], t=r["cand"][chosen][1], good=good, chosen=chosen, n_inliers=good[chosen], masks=masks, mask=masks[chosen].copy())


def invert_pose(R, T):
    """Rotation = R', Translation = -R' T"""
    return [[R[j][i] for j in range(3)] for i in range(3)], [((-R[0][i]) * T[0] + (-R[1][i]) * T[1]) + (-R[2][i]) * T[2] for i in range(3)]


def average_parallax(pairs):
    s = 0.0
    for p in pairs:
        dx, dy = float(p[0]) - float(p[3]), float(p[1]) - float(p[4])
        s = s + math.sqrt(dx * dx + dy * dy)
    return 1.0 * s / len(pairs)


def pair_points(pairs):
    pairs = np.asarray(pairs, np.float64).reshape(-1, 6)
    return pairs[:, 0:2].astype(np.float32), pairs[:, 3:5].astype(np.float32)


def solve_relative_rt(pairs, threshold=THRESHOLD, confidence=CONFIDENCE, dist=DIST, max_iters=1000, model=None):
    """MotionEstimator::solveRelativeRT -> dict(ok, Rotation, Translation, flags, pose, status, F).  model: (status, F,
    best_iter) to use in place of fmat_ref.find: the device's own model, which agrees with the reference's only to
    rounding."""
    pairs = np.asarray(pairs, np.float64).reshape(-1, 6)
    n = len(pairs)
    eye = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    out = dict(ok=False, Rotation=eye, Translation=[0.0] * 3, flags=0, pose=None, status=np.zeros(n, np.uint8), F=np.zeros((3, 3)))
    if n < MIN_PAIRS_SOLVE:
        out["flags"] = FLAG_TOO_FEW
        return out
    p1, p2 = pair_points(pairs)
    if model is None:
        status, tr = fmat_ref.find(p1, p2, threshold, confidence, max_iters)
        model = (status, tr["F_best"], tr["best_iter"])
    status, F, best_iter = model
    out["status"], out["F"] = np.asarray(status, np.uint8), np.asarray(F, np.float64).reshape(3, 3)
    if best_iter < 0:
        out["flags"] = FLAG_NO_MODEL
        return out
    pose = recover(F, p1, p2, status, dist)
    out["pose"], out["flags"] = pose, pose["flags"]
    out["Rotation"], out["Translation"] = invert_pose(pose["R"], pose["t"])
    out["ok"] = pose["n_inliers"] > MIN_INLIERS
    return out


def relative_pose(corresponding, solve=solve_relative_rt):
    """Estimator::relativePose: corresponding(i, WINDOW) -> pairs [n][6] -> (ok, l, Rotation, Translation, records).  A
    failed solve has still overwritten Rotation and Translation; only ok says whether they mean anything."""
    eye = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    R, T, records = eye, [0.0] * 3, []
    for i in range(WINDOW):
        pairs = np.asarray(corresponding(i, WINDOW), np.float64).reshape(-1, 6)
        rec = dict(frame=i, n=len(pairs), average_parallax=None, solved=False, ok=False)
        records.append(rec)
        if len(pairs) > MIN_PAIRS_GATE:
            rec["average_parallax"] = average_parallax(pairs)
            if rec["average_parallax"] * FOCAL > MIN_PARALLAX_PX:
                s = solve(pairs)
                rec.update(solved=True, ok=s["ok"], result=s)
                R, T = s["Rotation"], s["Translation"]
                if s["ok"]:
                    return True, i, R, T, records
    return False, -1, R, T, records


# ---- mpmath ---------------------------------------------------------------------------------------------------------------
def candidates_mp(E):
    """the four candidates at MP_DIGITS digits -> list of (R mp.matrix, t mp.matrix)"""
    with mp.workdps(MP_DIGITS):
        U, S, Vt = mp.svd_r(mp.matrix(np.asarray(E, np.float64).reshape(3, 3).tolist()))
        if mp.det(U) < 0:
            U = -U
        if mp.det(Vt) < 0:
            Vt = -Vt
        W = mp.matrix([[0, 1, 0], [-1, 0, 0], [0, 0, 1]])
        R1, R2, t = U * W * Vt, U * W.T * Vt, U[:, 2]
        return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def pose_dev(R, t, cands):
    """the distance of a float64 pose from the nearest of the exact candidates: largest absolute entry difference"""
    with mp.workdps(MP_DIGITS):
        best = None
        for Rm, tm in cands:
            d = max([abs(mp.mpf(R[i][j]) - Rm[i, j]) for i in range(3) for j in range(3)] + [abs(mp.mpf(t[i]) - tm[i]) for i in range(3)])
            best = d if best is None or d < best else best
        return float(best)


def pose_bar(G):
    """§26's bar: 10 G, never below 16 ulp"""
    return max(10.0 * G, 16 * 2.0 ** -52)


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


def motion(seed):
    rs = np.random.RandomState(1000 + seed)
    R = fmat_ref.rot(*rs.uniform(-0.25, 0.25, 3))
    t = rs.uniform(-1, 1, 3)
    t = t / np.linalg.norm(t) * rs.uniform(0.3, 1.0)
    return R, t


def two_view(seed, n=60, noise=0.0, outliers=0.0):
    """x2 = R x1 + t on the normalised plane: (pts1, pts2 [n, 2] float32, R, t, E = [t]x R, depths in view 0)"""
    R, t = motion(seed)
    rs = np.random.RandomState(seed)
    xy = np.c_[rs.uniform(-0.7, 0.7, n), rs.uniform(-0.45, 0.45, n)]
    Z = rs.uniform(2, 20, n)
    X = np.c_[xy, np.ones(n)] * Z[:, None]
    X2 = X @ R.T + t
    p2 = X2[:, :2] / X2[:, 2:3]
    if noise > 0:
        p2 = p2 + rs.normal(0, noise, p2.shape)
    k = int(round(outliers * n))
    if k:
        bad = rs.choice(n, k, replace=False)
        p2[bad] += rs.uniform(15, 60, (k, 2)) / FOCAL * rs.choice([-1, 1], (k, 2))
    return xy.astype(np.float32), p2.astype(np.float32), R, t, skew(t) @ R, Z


def pairs_of(p1, p2):
    """getCorresponding's pairs [n][6] from two point sets (z = 1)"""
    n = len(p1)
    return np.c_[np.asarray(p1, np.float64), np.ones(n), np.asarray(p2, np.float64), np.ones(n)]


EXACT_SEEDS = tuple(range(12))
F_SEEDS = tuple(range(20, 28))
_scene_cache = {}


def scenes():
    """name -> dict(E, p1, p2, mask, R, t): exact essential matrices, and 7-point F matrices of the same kind of points with
    1 / 460 noise from fmat_ref, with its status as the mask.  Computed once per process and never changed."""
    if not _scene_cache:
        for s in EXACT_SEEDS:
            p1, p2, R, t, E, _ = two_view(s, 40 + 7 * s)
            _scene_cache[f"exact{s}"] = dict(E=E, p1=p1, p2=p2, mask=None, R=R, t=t)
        for s in F_SEEDS:
            p1, p2, R, t, E, _ = two_view(s, 90, noise=1.0 / FOCAL)
            status, tr = fmat_ref.find(p1, p2, THRESHOLD, CONFIDENCE, 1000)
            assert tr["best_iter"] >= 0
            _scene_cache[f"fmat{s}"] = dict(E=np.array(tr["F_best"]), p1=p1, p2=p2, mask=status, R=R, t=t)
    return _scene_cache


def frames_from_tracks(tracks):
    """tracks: per feature (start frame, [(x, y) of frames start .. WINDOW]) -> the eleven (ids, obs [n][8]) a feature manager
    is loaded with (fman_ref.load); a feature's id is its index"""
    frames = [([], []) for _ in range(WINDOW + 1)]
    for fid, (start, xy) in enumerate(tracks):
        assert start + len(xy) == WINDOW + 1
        for o, (x, y) in enumerate(xy):
            frames[start + o][0].append(fid)
            frames[start + o][1].append([float(x), float(y), 1.0, FOCAL * float(x) + 320.0, FOCAL * float(y) + 240.0, 0.0, 0.0, -1.0])
    return frames


def _track(start, first, last, still=0):
    """observations from `first` (frame start) to `last` (frame WINDOW) on a straight line; the first `still` frames stay
    within 1e-3 of `last`: a parallax of half a pixel"""
    k = WINDOW - start
    xy = [(first[0] + (last[0] - first[0]) * o / k, first[1] + (last[1] - first[1]) * o / k) for o in range(k + 1)]
    for o in range(still):
        xy[o] = (last[0] + 1e-3, last[1])
    return start, xy


def pure_translation(seed, n, target):
    """x2 = x1 + s / Z, y2 = y1 (R = I, t along x), s chosen so that average_parallax comes out at `target`"""
    rs = np.random.RandomState(seed)
    p1 = np.c_[rs.uniform(-0.7, 0.7, n), rs.uniform(-0.45, 0.45, n)]
    inv_z = 1.0 / rs.uniform(2, 20, n)
    s = 1.0
    for _ in range(4):
        p2 = p1 + np.c_[s * inv_z, np.zeros(n)]
        s = s * target / average_parallax(pairs_of(p1, p2))
    return p1, p1 + np.c_[s * inv_z, np.zeros(n)]


WINDOWS = ("first", "third", "garbage", "still", "pairs20", "pairs21", "below", "above")


def window_frames(kind, seed=5, n=40):
    """the windows of relativePose -> the eleven frames of frames_from_tracks.
    first: frame 0 passes.  third: 25 features start at frame 0 and do not move before frame 3, where 15 more start:
    frames 0..2 fail on parallax, frame 3 passes.  garbage: the same, but the 25 early features jump about in frames 0..2: the
    solve runs there, fails, and has overwritten R and T.  still: no feature moves, none passes.  pairs20 / pairs21: that many
    features, all from frame 0: the gate wants more than 20.  below / above: a pure translation whose average parallax
    is 30 pixels x (1 -+ 1e-9)."""
    if kind in ("below", "above"):
        p1, p2 = pure_translation(seed, n, MIN_PARALLAX_PX / FOCAL * (1 - 1e-9 if kind == "below" else 1 + 1e-9))
        return frames_from_tracks([_track(0, a, b) for a, b in zip(p1, p2)])
    p1, p2, *_ = two_view(100 + seed, n)
    p1, p2 = p1.astype(np.float64), p2.astype(np.float64)
    if kind == "first":
        tracks = [_track(0, a, b) for a, b in zip(p1, p2)]
    elif kind == "third":
        tracks = [_track(0, a, b, still=3) if k < 25 else _track(3, a, b) for k, (a, b) in enumerate(zip(p1, p2))]
        for k in range(25):                                   # frame 3 of an early feature is the scene's first view
            tracks[k][1][3] = (p1[k][0], p1[k][1])
    elif kind == "garbage":
        rs = np.random.RandomState(seed)
        tracks = [_track(0, a, b) if k < 25 else _track(3, a, b) for k, (a, b) in enumerate(zip(p1, p2))]
        for k in range(25):
            tracks[k][1][:4] = [(rs.uniform(-0.7, 0.7), rs.uniform(-0.45, 0.45)) for _ in range(3)] + [(p1[k][0], p1[k][1])]
    elif kind == "still":
        tracks = [_track(0, a, b, still=WINDOW) for a, b in zip(p1, p2)]
    else:
        m = 20 if kind == "pairs20" else 21
        tracks = [_track(0, a, b) for a, b in zip(p1[:m], p2[:m])]
    return frames_from_tracks(tracks)


def planted(seed=40, n=24):
    """R = I, t = (1, 0, 0) s: E, U, V and both rotations come out exact, so what is planted stays exact.  Point 0 is the
    origin in both views: parallel rays, column 2 of its 4 x 4 matrix is exactly zero and Q = (0, 0, 1, 0), Q3 == 0.
    Point 1 lies at 80 baselines (beyond the distance threshold), point 2 at 40."""
    rs = np.random.RandomState(seed)
    s = 0.5
    xy = np.c_[rs.uniform(-0.7, 0.7, n), rs.uniform(-0.45, 0.45, n)]
    Z = rs.uniform(2, 20, n)
    Z[1], Z[2] = 80 * s, 40 * s
    X = np.c_[xy, np.ones(n)] * Z[:, None]
    X2 = X + np.array([s, 0, 0])
    p2 = X2[:, :2] / X2[:, 2:3]
    xy[0], p2[0] = 0.0, 0.0
    E = skew([1.0, 0.0, 0.0])
    return dict(E=E, p1=xy.astype(np.float32), p2=p2.astype(np.float32), mask=None, dist=DIST)


def tie(seed=41, k=9):
    """k points of the motion (R, t) and k of (R, -t), which share E: two candidates count k each"""
    a1, a2, R, t, E, _ = two_view(seed, k)
    rs = np.random.RandomState(seed + 1)
    xy = np.c_[rs.uniform(-0.7, 0.7, k), rs.uniform(-0.45, 0.45, k)]
    X = np.c_[xy, np.ones(k)] * rs.uniform(2, 8, k)[:, None]
    X2 = X @ R.T - t
    b2 = X2[:, :2] / X2[:, 2:3]
    return dict(E=E, p1=np.r_[a1, xy.astype(np.float32)], p2=np.r_[a2, b2.astype(np.float32)], mask=None, dist=DIST)


def branch_scenes():
    """name -> dict(E, p1, p2, mask, dist): the branches of recoverPose"""
    out = {"planted": planted(), "tie": tie()}
    p1, p2, R, t, E, _ = two_view(7, 30)
    base = dict(E=E, p1=p1, p2=p2, mask=None, dist=DIST)
    out["zero_mask"] = dict(base, mask=np.zeros(30, np.uint8))
    out["near"] = dict(base, dist=12.0)
    out["E_zero"] = dict(base, E=np.zeros((3, 3)))
    out["E_rank1"] = dict(base, E=np.array([[0.0, 2.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]))
    out["E_outer"] = dict(base, E=np.outer([0.3, -0.2, 0.9], [0.5, 0.1, -0.7]))
    nan = E.copy()
    nan[1, 2] = NAN
    out["E_nan"] = dict(base, E=nan)
    inf = E.copy()
    inf[0, 0] = math.inf
    out["E_inf"] = dict(base, E=inf)
    out["E_huge"] = dict(base, E=E * 1e200)
    out["E_neg"] = dict(base, E=-E)
    out["E_small"] = dict(base, E=1e-3 * E)
    return out


def inlier_scene(k, n=30, seed=44):
    """an exact scene and a mask with exactly k ones among points every one of which passes the winner -> pairs, status, E"""
    p1, p2, R, t, E, Z = two_view(seed, n)
    full = recover(E, p1, p2)
    keep = np.flatnonzero(full["mask"])[:k]
    assert len(keep) == k
    status = np.zeros(n, np.uint8)
    status[keep] = 1
    return pairs_of(p1, p2), status, E
