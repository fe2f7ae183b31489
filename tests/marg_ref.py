"""Reference of the sliding-window marginalisation (include/lvi_marg.h): a restatement of
projection_factor.cpp:21-121, projection_td_factor.cpp:34-141, ResidualBlockInfo::Evaluate and MarginalizationInfo
(marginalization_factor.cpp:37-68, 89-129, 174-318), MarginalizationFactor::Evaluate (:332-380) and the two branches of
estimator.cpp:813-976, in two arithmetics from the same float64 inputs: numpy float64 (`F64`, eigh by LAPACK) and mpmath
at 50 digits (`MP`, eigsy).  G, the distance between the two, is the reference's own error; the GPU tier derives its
tolerances from it.  Nothing here reads the library."""
import math

import mpmath
import numpy as np

mpmath.mp.dps = 50
EPS = 1e-8
FOCAL_LENGTH, WINDOW_SIZE = 460.0, 10
SQRT_INFO = FOCAL_LENGTH / 1.5
LOSS_NONE, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2
DBL_MIN = 2.2250738585072014e-308


class Arith:
    """the scalar type and the handful of functions the restatement needs"""

    def __init__(self, name):
        self.name, self.mp = name, name == "mp"
        self.dtype = object if self.mp else np.float64

    def num(self, x):
        return mpmath.mpf(float(x)) if self.mp and not isinstance(x, mpmath.mpf) else (x if self.mp else float(x))

    def arr(self, a):
        a = np.asarray(a, dtype=object if self.mp else np.float64)
        return np.vectorize(self.num, otypes=[object])(a) if self.mp and a.size else a

    def zeros(self, *shape):
        z = np.zeros(shape, self.dtype)
        if self.mp:
            z[...] = mpmath.mpf(0)
        return z

    def sqrt(self, x):
        return mpmath.sqrt(x) if self.mp else math.sqrt(x)

    def log(self, x):
        return mpmath.log(x) if self.mp else math.log(x)

    def eigh(self, A):
        """ascending eigenvalues and eigenvectors (columns) of a symmetric matrix"""
        if not self.mp:
            return np.linalg.eigh(A)
        n = A.shape[0]
        E, Q = mpmath.eigsy(mpmath.matrix(A.tolist()))
        w = np.array([E[i] for i in range(n)], object)
        V = np.array([[Q[i, j] for j in range(n)] for i in range(n)], object).reshape(n, n)
        o = sorted(range(n), key=lambda i: w[i])
        return w[o], V[:, o]


    def eigvals(self, A):
        if not self.mp:
            return np.linalg.eigvalsh(A)
        E = mpmath.eigsy(mpmath.matrix(A.tolist()), eigvals_only=True)
        return np.array(sorted(E[i] for i in range(A.shape[0])), object)


F64, MP = Arith("f64"), Arith("mp")
EXACT_ZERO = 1e-30               # an mpmath eigenvalue below this fraction of the largest is an exact zero


def psd_factor(H, g, X):
    """J [n, n] (zero rows below the rank) and r with J'J = H, J'r = g for a positive semi-definite H with g in its range:
    outer-product Cholesky with diagonal pivoting, at the precision of X"""
    n = H.shape[0]
    W, J, r, piv = H.copy(), X.zeros(n, n), X.zeros(n), []
    top = max(W[i, i] for i in range(n))
    for k in range(n):
        p = max(range(n), key=lambda i: W[i, i])
        if not W[p, p] > EXACT_ZERO * top:
            break
        v = W[:, p] / X.sqrt(W[p, p])
        J[k] = v
        W = W - np.outer(v, v)
        piv.append(p)
        r[k] = (g[p] - sum(J[j, p] * r[j] for j in range(k))) / J[k, p]
    return J, r


def to_f64(a):
    return np.array(a, dtype=np.float64) if not np.isscalar(a) else float(a)


# ---- factors ---------------------------------------------------------------------------------------------
def quat_to_rot(q, X):
    x, y, z, w = q
    two = X.num(2.0)
    one = X.num(1.0)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], X.dtype)


def skew(v, X):
    z = X.num(0.0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], X.dtype)


def projection_eval(pose_i, pose_j, ex, inv_dep, td, use_td, obs, X, sqrt_info=SQRT_INFO, tr_over_row=0.0, half_row=240.0):
    """obs: dict(pts_i, pts_j, velocity_i, velocity_j, td_i, td_j, row_i, row_j) -> (r [2], J [2, 20]): columns pose_i 0..5,
    pose_j 6..11, extrinsic 12..17, inverse depth 18, td 19 (zero for ProjectionFactor)"""
    A = X.arr
    pose_i, pose_j, ex = A(pose_i), A(pose_j), A(ex)
    inv_dep, td, si = X.num(inv_dep), X.num(td), X.num(sqrt_info)
    Pi, Pj, tic = pose_i[:3], pose_j[:3], ex[:3]
    Ri, Rj, ric = quat_to_rot(pose_i[3:7], X), quat_to_rot(pose_j[3:7], X), quat_to_rot(ex[3:7], X)
    pts_i, pts_j = A(obs["pts_i"]), A(obs["pts_j"])
    vi, vj = A(list(obs["velocity_i"]) + [0.0]), A(list(obs["velocity_j"]) + [0.0])
    if use_td:
        ki = td - X.num(obs["td_i"]) + X.num(tr_over_row) * (X.num(obs["row_i"]) - X.num(half_row))
        kj = td - X.num(obs["td_j"]) + X.num(tr_over_row) * (X.num(obs["row_j"]) - X.num(half_row))
        pts_i_td, pts_j_td = pts_i - ki * vi, pts_j - kj * vj
    else:
        pts_i_td, pts_j_td = pts_i, pts_j
    pc_i = pts_i_td / inv_dep
    p_imu_i = ric @ pc_i + tic
    p_w = Ri @ p_imu_i + Pi
    p_imu_j = Rj.T @ (p_w - Pj)
    pc_j = ric.T @ (p_imu_j - tic)
    dep_j = pc_j[2]
    r = si * (pc_j[:2] / dep_j - pts_j_td[:2])
    one, z = X.num(1.0), X.num(0.0)
    reduce = si * np.array([[one / dep_j, z, -pc_j[0] / (dep_j * dep_j)], [z, one / dep_j, -pc_j[1] / (dep_j * dep_j)]], X.dtype)
    J = X.zeros(2, 20)
    J[:, 0:3] = reduce @ (ric.T @ Rj.T)
    J[:, 3:6] = reduce @ (ric.T @ Rj.T @ Ri @ (-skew(p_imu_i, X)))
    J[:, 6:9] = reduce @ (ric.T @ (-Rj.T))
    J[:, 9:12] = reduce @ (ric.T @ skew(p_imu_j, X))
    eye = X.arr(np.eye(3))
    tmp_r = ric.T @ Rj.T @ Ri @ ric
    J[:, 12:15] = reduce @ (ric.T @ (Rj.T @ Ri - eye))
    J[:, 15:18] = reduce @ (-tmp_r @ skew(pc_i, X) + skew(tmp_r @ pc_i, X) + skew(ric.T @ (Rj.T @ (Ri @ tic + Pi - Pj) - tic), X))
    J[:, 18] = reduce @ (tmp_r @ pts_i_td) * (-one) / (inv_dep * inv_dep)
    if use_td:
        J[:, 19] = reduce @ (tmp_r @ vi) / inv_dep * (-one) + si * vj[:2]
    return r, J


def loss_rho(kind, a, s, X):
    """ceres::CauchyLoss(a) / HuberLoss(a)::Evaluate"""
    a = X.num(a)
    b = a * a
    one = X.num(1.0)
    if kind == LOSS_CAUCHY:
        c = one / b
        inv = one / (one + s * c)
        return [b * X.log(one + s * c), max(inv, X.num(DBL_MIN)), -c * (inv * inv)]
    if kind == LOSS_HUBER and s > b:
        rt = X.sqrt(s)
        r1 = max(a / rt, X.num(DBL_MIN))
        return [X.num(2.0) * a * rt - b, r1, -r1 / (X.num(2.0) * s)]
    return [s, one, X.num(0.0)]


def loss_correct(r, J, rho, X):
    """marginalization_factor.cpp:37-68 as written, both branches -> (r, J)"""
    sq_norm = sum(x * x for x in r)
    sqrt_rho1 = X.sqrt(rho[1])
    one = X.num(1.0)
    if sq_norm == 0 or rho[2] <= 0:
        residual_scaling, alpha_sq_norm = sqrt_rho1, X.num(0.0)
    else:
        D = one + X.num(2.0) * sq_norm * rho[2] / rho[1]
        alpha = one - X.sqrt(D)
        residual_scaling, alpha_sq_norm = sqrt_rho1 / (one - alpha), alpha / sq_norm
    r = np.asarray(r, X.dtype)
    J = sqrt_rho1 * (J - alpha_sq_norm * np.outer(r, r @ J))
    return r * residual_scaling, J


def local_size(size):
    return 6 if size == 7 else size


def prior_dx(size, x, x0, X):
    """:349-361; Utility::positify returns its argument (utility.h:41-48), so the sign branch is what fixes the sign"""
    x, x0 = X.arr(x), X.arr(x0)
    if size != 7:
        return x - x0
    n2 = sum(v * v for v in x0[3:7])
    a = np.array([-x0[3] / n2, -x0[4] / n2, -x0[5] / n2, x0[6] / n2], X.dtype)          # q0.inverse(), x y z w
    b = x[3:7]
    w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
    v = np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                  a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                  a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0]], X.dtype)
    two = X.num(2.0)
    dq = two * v if w >= 0 else two * (-v)
    return np.concatenate([x[:3] - x0[:3], dq])


# ---- MarginalizationInfo ------------------------------------------------------------------------------------
class Marg:
    """one marginalisation in arithmetic X.  Blocks are named by ids; the order is the library's: dropped blocks by first
    appearance in a drop set, kept blocks by first appearance; a block no factor names is left out."""

    def __init__(self, X, loss=LOSS_CAUCHY, loss_a=1.0, sqrt_info=SQRT_INFO, tr_over_row=0.0, half_row=240.0, eps=EPS):
        self.X, self.loss, self.loss_a, self.eps = X, loss, loss_a, eps
        self.const = dict(sqrt_info=sqrt_info, tr_over_row=tr_over_row, half_row=half_row)
        self.blocks, self.order_decl, self.seen, self.drop, self.seq = {}, [], {}, {}, 0
        self.factors = []                      # (ids, r, [J per block, local columns])

    def set_block(self, bid, values):
        if bid not in self.blocks:
            self.order_decl.append(bid)
        self.blocks[bid] = np.array(values, np.float64)

    def _appear(self, bid, drop):
        self.seen.setdefault(bid, self.seq)
        if drop:
            self.drop.setdefault(bid, self.seq)
        self.seq += 1

    def add_projection(self, rec):
        """rec: dict(pose_i, pose_j, ex, feature, td (or -1), pts_i, ...)"""
        X = self.X
        use_td = rec["td"] != -1
        ids = [rec["pose_i"], rec["pose_j"], rec["ex"], rec["feature"]] + ([rec["td"]] if use_td else [])
        td = self.blocks[rec["td"]][0] if use_td else 0.0
        r, J = projection_eval(self.blocks[ids[0]], self.blocks[ids[1]], self.blocks[ids[2]], self.blocks[ids[3]][0], td, use_td, rec, X, **self.const)
        if self.loss != LOSS_NONE:
            r, J = loss_correct(r, J, loss_rho(self.loss, self.loss_a, sum(x * x for x in r), X), X)
        Js = [J[:, 0:6], J[:, 6:12], J[:, 12:18], J[:, 18:19]] + ([J[:, 19:20]] if use_td else [])
        for k, b in enumerate(ids):
            self._appear(b, k in (0, 3))
        self.factors.append((ids, r, Js))

    def add_dense(self, ids, residual, jacobians, drop):
        X = self.X
        Js = [X.arr(np.asarray(j, np.float64).reshape(len(residual), -1)[:, :local_size(len(self.blocks[b]))]) for j, b in zip(jacobians, ids)]
        for b, d in zip(ids, drop):
            self._appear(b, bool(d))
        self.factors.append((list(ids), X.arr(residual), Js))

    def add_prior(self, prior, drop_ids):
        """prior: the dict a marginalize() of this arithmetic returned (its ids possibly remapped)"""
        X = self.X
        n = prior["n"]
        dx = X.zeros(n)
        for bid, size, col, x0 in zip(prior["ids"], prior["sizes"], prior["col"], prior["x0"]):
            dx[col:col + local_size(size)] = prior_dx(size, self.blocks[bid], x0, X)
        r = prior["r"] + prior["J"] @ dx
        Js = [prior["J"][:, c:c + local_size(s)] for c, s in zip(prior["col"], prior["sizes"])]
        for b in prior["ids"]:
            self._appear(b, b in list(drop_ids))
        self.factors.append((list(prior["ids"]), r, Js))

    def layout(self):
        dropped = sorted(self.drop, key=lambda b: self.drop[b])
        kept = sorted((b for b in self.seen if b not in self.drop), key=lambda b: self.seen[b])
        col, pos = {}, 0
        for b in dropped + kept:
            col[b] = pos
            pos += local_size(len(self.blocks[b]))
            if b in self.drop:
                m = pos
        return dropped, kept, col, m, pos - m

    def system(self):
        X = self.X
        _, _, col, m, n = self.layout()
        A, b = X.zeros(m + n, m + n), X.zeros(m + n)
        for ids, r, Js in self.factors:
            for bi, Ji in zip(ids, Js):
                ci, si = col[bi], Ji.shape[1]
                for bj, Jj in zip(ids, Js):
                    A[ci:ci + si, col[bj]:col[bj] + Jj.shape[1]] += Ji.T @ Jj
                b[ci:ci + si] += Ji.T @ r
        return A, b, m, n

    def marginalize(self):
        """:174-296 -> dict(A, b, m, n, w_mm, w_rr, H, g, Hp, gp, J, r, rank, ids, sizes, col, x0)"""
        X, eps = self.X, self.eps
        A, b, m, n = self.system()
        _, kept, col, _, _ = self.layout()
        half = X.num(0.5)
        Amm = half * (A[:m, :m] + A[:m, :m].T)
        w, V = X.eigh(Amm)
        one = X.num(1.0)
        winv = np.array([one / x if x > eps else X.num(0.0) for x in w], X.dtype)
        Amm_inv = (V * winv) @ V.T
        H = A[m:, m:] - A[m:, :m] @ Amm_inv @ A[:m, m:]
        g = b[m:] - A[m:, :m] @ Amm_inv @ b[:m]
        if X.mp:
            Hs = half * (H + H.T)
            w2 = X.eigvals(Hs)
            if not any(EXACT_ZERO * max(abs(x) for x in w2) < x <= eps for x in w2):
                # no eigenvalue between an exact zero and eps: thresholding drops nothing but exact zeros, so any J with
                # J'J = H and J'r = g is the prior up to an orthogonal transform of its rows, which no comparison sees
                J, r = psd_factor(Hs, g, X)
                return dict(A=A, b=b, m=m, n=n, w_mm=w, w_rr=w2, H=H, g=g, Hp=Hs, gp=g, J=J, r=r, rank=int(sum(1 for x in w2 if x > eps)), ids=list(kept),
                            sizes=[len(self.blocks[k]) for k in kept], col=[col[k] - m for k in kept], x0=[self.blocks[k].copy() for k in kept])
            w2, V2 = X.eigh(Hs)
        else:
            w2, V2 = X.eigh(H)
        S = np.array([x if x > eps else X.num(0.0) for x in w2], X.dtype)
        S_inv = np.array([one / x if x > eps else X.num(0.0) for x in w2], X.dtype)
        J = (V2 * np.array([X.sqrt(x) for x in S], X.dtype)).T
        r = np.array([X.sqrt(x) for x in S_inv], X.dtype) * (V2.T @ g)
        # Hp, gp: what the prior holds, J'J and J'r: the Schur complement without what the threshold dropped.  An eigenvalue
        # lambda <= eps that is not an exact zero takes lambda out of H and (v'g) v out of g, in the reference as here.
        return dict(A=A, b=b, m=m, n=n, w_mm=w, w_rr=w2, H=H, g=g, Hp=J.T @ J, gp=J.T @ r, J=J, r=r, rank=int(sum(1 for x in w2 if x > eps)), ids=list(kept),
                    sizes=[len(self.blocks[k]) for k in kept], col=[col[k] - m for k in kept], x0=[self.blocks[k].copy() for k in kept])


def remap(prior, old_ids, new_ids):
    t = dict(zip(old_ids, new_ids))
    out = dict(prior)
    out["ids"] = [t.get(b, b) for b in prior["ids"]]
    return out


# ---- the two branches of estimator.cpp:813-976 -----------------------------------------------------------------
MARGIN_OLD, MARGIN_SECOND_NEW = 0, 1
ID_POSE, ID_SPEEDBIAS, ID_EX, ID_TD, ID_FEATURE = 0, 16, 32, 33, 64       # the host mirror's ids: pose k, speed-bias k, ...


def declare_window(M, win):
    for k in range(WINDOW_SIZE + 1):
        M.set_block(ID_POSE + k, win["pose"][k])
        M.set_block(ID_SPEEDBIAS + k, win["speed_bias"][k])
    M.set_block(ID_EX, win["ex"])
    M.set_block(ID_TD, [win["td"]])


def vins_projections(win, features, estimate_td):
    """:847-890 -> the records of MARGIN_OLD, and the feature blocks they need {id: inverse depth}"""
    recs, blocks, feature_index = [], {}, -1
    for f in features:
        used = len(f["obs"])
        if not (used >= 2 and f["start_frame"] < WINDOW_SIZE - 2):
            continue
        feature_index += 1
        imu_i, imu_j = f["start_frame"], f["start_frame"] - 1
        if imu_i != 0:
            continue
        o0 = f["obs"][0]
        for o in f["obs"]:
            imu_j += 1
            if imu_i == imu_j:
                continue
            blocks[ID_FEATURE + feature_index] = f["inv_dep"]
            recs.append(dict(pose_i=ID_POSE + imu_i, pose_j=ID_POSE + imu_j, ex=ID_EX, feature=ID_FEATURE + feature_index, td=ID_TD if estimate_td else -1,
                             pts_i=o0["point"], pts_j=o["point"], velocity_i=o0["velocity"], velocity_j=o["velocity"], td_i=o0["cur_td"], td_j=o["cur_td"],
                             row_i=o0["uv_y"], row_j=o["uv_y"]))
    return recs, blocks


def vins_marginalize(X, prior, flag, win, features=(), imu=None, estimate_td=True, **kw):
    """one pass through :813-976 in arithmetic X -> the new prior (ids already shifted), or `prior` itself when the branch
    does nothing.  imu: None (sum_dt >= 10, or no factor) or dict(residual [15], jacobians [4])."""
    M = Marg(X, **kw)
    declare_window(M, win)
    if flag == MARGIN_OLD:
        if prior is not None:
            M.add_prior(prior, [b for b in prior["ids"] if b in (ID_POSE, ID_SPEEDBIAS)])
        if imu is not None:
            M.add_dense([ID_POSE, ID_SPEEDBIAS, ID_POSE + 1, ID_SPEEDBIAS + 1], imu["residual"], imu["jacobians"], [1, 1, 0, 0])
        recs, fblocks = vins_projections(win, features, estimate_td)
        for bid, v in fblocks.items():
            M.set_block(bid, [v])
        for rec in recs:
            M.add_projection(rec)
        out = M.marginalize()
        old = [ID_POSE + i for i in range(1, WINDOW_SIZE + 1)] + [ID_SPEEDBIAS + i for i in range(1, WINDOW_SIZE + 1)]
        return remap(out, old, [b - 1 for b in old])
    if prior is None or ID_POSE + WINDOW_SIZE - 1 not in prior["ids"]:
        return prior
    M.add_prior(prior, [ID_POSE + WINDOW_SIZE - 1])
    out = M.marginalize()
    return remap(out, [ID_POSE + WINDOW_SIZE, ID_SPEEDBIAS + WINDOW_SIZE], [ID_POSE + WINDOW_SIZE - 1, ID_SPEEDBIAS + WINDOW_SIZE - 1])


# ---- scenes ----------------------------------------------------------------------------------------------------
def rand_quat(rs, scale):
    w = rs.normal(0, scale, 3)
    th = np.linalg.norm(w)
    q = np.r_[np.sin(th / 2) * w / max(th, 1e-300), np.cos(th / 2)]
    return q / np.linalg.norm(q)


def quat_mul(a, b):
    av, bv = a[:3], b[:3]
    return np.r_[a[3] * bv + b[3] * av + np.cross(av, bv), a[3] * b[3] - av @ bv]


def rot(q):
    return quat_to_rot(np.asarray(q, np.float64), F64)


def make_window(seed, n_features, frames_seen=None, noise_px=0.5, first_frames=(0,)):
    """a window of WINDOW_SIZE + 1 poses moving forward, a camera looking ahead, features 4..12 m away; every feature is
    seen from its start frame over frames_seen consecutive frames.  Observations are exact projections plus noise_px of
    pixel noise; the stored inverse depths and poses are perturbed, so the residuals are not zero."""
    rs = np.random.RandomState(seed)
    pose = np.zeros((WINDOW_SIZE + 1, 7))
    for k in range(WINDOW_SIZE + 1):
        pose[k, :3] = [0.3 * k + rs.normal(0, 0.02), rs.normal(0, 0.05), rs.normal(0, 0.02)]
        pose[k, 3:] = rand_quat(rs, 0.05)
    sb = rs.normal(0, 0.1, (WINDOW_SIZE + 1, 9))
    # camera z forward = body x: ric columns = camera axes in the body frame
    ric = np.array([[0., 0., 1.], [-1., 0., 0.], [0., -1., 0.]])
    qw = math.sqrt(1 + ric[0, 0] + ric[1, 1] + ric[2, 2]) / 2
    q = np.array([(ric[2, 1] - ric[1, 2]) / (4 * qw), (ric[0, 2] - ric[2, 0]) / (4 * qw), (ric[1, 0] - ric[0, 1]) / (4 * qw), qw])
    ex = np.r_[0.05, -0.02, 0.03, quat_mul(q, rand_quat(rs, 0.02))]
    ex[3:] /= np.linalg.norm(ex[3:])
    td = 0.01
    Rc, feats = rot(ex[3:]), []
    for f in range(n_features):
        start = first_frames[f % len(first_frames)]
        seen = frames_seen[f % len(frames_seen)] if frames_seen else WINDOW_SIZE + 1 - start
        Ri = rot(pose[start, 3:])
        depth = rs.uniform(4, 12)
        pc = np.r_[rs.uniform(-0.4, 0.4), rs.uniform(-0.3, 0.3), 1.0] * depth
        pw = Ri @ (Rc @ pc + ex[:3]) + pose[start, :3]
        obs = []
        for j in range(start, min(start + seen, WINDOW_SIZE + 1)):
            pj = Rc.T @ (rot(pose[j, 3:]).T @ (pw - pose[j, :3]) - ex[:3])
            uv = pj[:2] / pj[2] + rs.normal(0, noise_px / FOCAL_LENGTH, 2)
            obs.append(dict(point=np.r_[uv, 1.0], velocity=rs.normal(0, 0.3, 2), cur_td=td + rs.normal(0, 1e-3), uv_y=float(240 + FOCAL_LENGTH * uv[1])))
        feats.append(dict(start_frame=start, inv_dep=float(1.0 / depth * (1 + rs.normal(0, 0.02))), obs=obs))
    return dict(pose=pose, speed_bias=sb, ex=ex, td=td), feats


def perturb_window(win, seed, scale=1e-2, flip=()):
    """changed parameter values for the next step of a chain; the quaternions of the poses in `flip` change sign"""
    rs = np.random.RandomState(seed)
    out = dict(pose=win["pose"].copy(), speed_bias=win["speed_bias"] + rs.normal(0, scale, win["speed_bias"].shape), ex=win["ex"].copy(),
               td=win["td"] + rs.normal(0, 1e-3))
    for k in range(WINDOW_SIZE + 1):
        out["pose"][k, :3] += rs.normal(0, scale, 3)
        out["pose"][k, 3:] = quat_mul(out["pose"][k, 3:], rand_quat(rs, scale))
        if k in flip:
            out["pose"][k, 3:] *= -1
    out["ex"][:3] += rs.normal(0, scale * 0.1, 3)
    out["ex"][3:] = quat_mul(out["ex"][3:], rand_quat(rs, scale * 0.1))
    return out


def shift_window(win, flag, seed):
    """slideWindow: MARGIN_OLD moves frame k + 1 to k, MARGIN_SECOND_NEW moves the newest frame to WINDOW_SIZE - 1; the
    newest frame is a fresh one"""
    rs = np.random.RandomState(seed)
    out = dict(pose=win["pose"].copy(), speed_bias=win["speed_bias"].copy(), ex=win["ex"].copy(), td=win["td"])
    if flag == MARGIN_OLD:
        out["pose"][:-1], out["speed_bias"][:-1] = win["pose"][1:], win["speed_bias"][1:]
    else:
        out["pose"][WINDOW_SIZE - 1], out["speed_bias"][WINDOW_SIZE - 1] = win["pose"][WINDOW_SIZE], win["speed_bias"][WINDOW_SIZE]
    out["pose"][WINDOW_SIZE, :3] += [0.3, rs.normal(0, 0.05), 0.0]
    out["pose"][WINDOW_SIZE, 3:] = quat_mul(out["pose"][WINDOW_SIZE, 3:], rand_quat(rs, 0.03))
    out["speed_bias"][WINDOW_SIZE] += rs.normal(0, 0.05, 9)
    return out


def imu_block(seed, info_max):
    """an IMU-like factor: 15 rows over (7, 9, 7, 9) with sqrt-information spread up to sqrt(info_max); not IMUFactor itself"""
    rs = np.random.RandomState(seed)
    sw = np.sqrt(np.logspace(2, np.log10(info_max), 15))
    Js = []
    for size in (7, 9, 7, 9):
        J = rs.normal(0, 1, (15, size)) * sw[:, None]
        if size == 7:
            J[:, 6] = 0.0
        Js.append(J)
    return dict(residual=rs.normal(0, 1, 15) * 0.1, jacobians=Js)


def gap(a, b):
    """largest |a - b| of two arrays of either arithmetic, as a float"""
    d = np.asarray(a, object) - np.asarray(b, object)
    return float(max((abs(x) for x in d.ravel()), default=0.0))


def norm2(a):
    a = to_f64(a)
    return float(np.linalg.norm(a, 2))


def scene_conditions(mp_out, eps=EPS):
    """the two conditions of a rank comparison -> (no exact eigenvalue inside [eps / 100, 100 eps], dim u ||A|| < eps / 10)"""
    ws = [float(x) for x in list(mp_out["w_mm"]) + list(mp_out["w_rr"])]
    clear = not any(eps / 100 <= x <= 100 * eps for x in ws)
    dim = mp_out["m"] + mp_out["n"]
    noise = dim * 2.2e-16 * norm2(mp_out["A"])
    return clear, noise < eps / 10, noise


# ---- the scenes of the GPU tier ------------------------------------------------------------------------------
# A scene is a script: params for Marg / the library, then ("block", id, values), ("proj", record), ("dense", ids, residual,
# jacobians, drop) in the order the caller would issue them.  `rank` says whether the scene is used for a rank comparison
# (tests/test_marg_ref.py asserts the two conditions of every such scene); the others are compared on H and g only.
def _rec(pi, pj, f, o0, o, td=ID_TD):
    return dict(pose_i=pi, pose_j=pj, ex=ID_EX, feature=f, td=td, pts_i=o0["point"], pts_j=o["point"], velocity_i=o0["velocity"], velocity_j=o["velocity"],
                td_i=o0["cur_td"], td_j=o["cur_td"], row_i=o0["uv_y"], row_j=o["uv_y"])


def _window_blocks(win, frames):
    ops = [("block", ID_POSE + k, win["pose"][k]) for k in frames]
    return ops + [("block", ID_EX, win["ex"]), ("block", ID_TD, [win["td"]])]


def _projection_scene(seed, frames_seen, use_td, count=None, outlier=None, params=None, rank=False):
    win, feats = make_window(seed, len(frames_seen), frames_seen=frames_seen)
    ops = _window_blocks(win, range(max(frames_seen)))
    recs = []
    for k, f in enumerate(feats):
        ops.append(("block", ID_FEATURE + k, [f["inv_dep"]]))
        for j in range(1, len(f["obs"])):
            recs.append(_rec(ID_POSE, ID_POSE + j, ID_FEATURE + k, f["obs"][0], f["obs"][j], ID_TD if use_td else -1))
    if outlier is not None:                                  # a 20-pixel error on one observation, so that the loss changes it
        r = dict(recs[outlier])
        r["pts_j"] = np.asarray(r["pts_j"], np.float64) + np.r_[20.0 / FOCAL_LENGTH, 0.0, 0.0]
        recs[outlier] = r
    recs = recs[:count] if count else recs
    used = {r["feature"] for r in recs}
    ops = [o for o in ops if not (o[0] == "block" and o[1] >= ID_FEATURE and o[1] not in used)]
    return dict(params=dict(params or {}), ops=ops + [("proj", r) for r in recs], rank=rank)


def _dense_scene(seed, drop_sizes, keep_sizes, rows, zero_block=None, rank=True):
    """one dense factor over blocks of the given sizes; the Jacobian of kept block `zero_block` is zero: no factor touches it"""
    rs = np.random.RandomState(seed)
    sizes = list(drop_sizes) + list(keep_sizes)
    ops, Js = [], []
    for k, s in enumerate(sizes):
        v = rs.normal(0, 1, s)
        if s == 7:
            v[3:] = rand_quat(rs, 0.3)
        ops.append(("block", 100 + k, v))
        J = rs.normal(0, 1, (rows, s))
        if s == 7:
            J[:, 6] = 0.0
        if zero_block is not None and k == len(drop_sizes) + zero_block:
            J[:] = 0.0
        Js.append(J)
    ops.append(("dense", [100 + k for k in range(len(sizes))], rs.normal(0, 1, rows), Js, [1] * len(drop_sizes) + [0] * len(keep_sizes)))
    return dict(params={}, ops=ops, rank=rank)


def _imu_scene(seed, info_max):
    sc = _projection_scene(seed, [4, 2, 3], True)
    win, _ = make_window(seed, 3, frames_seen=[4, 2, 3])
    ops = [("block", ID_SPEEDBIAS, win["speed_bias"][0]), ("block", ID_SPEEDBIAS + 1, win["speed_bias"][1])]
    imu = imu_block(seed + 1, info_max)
    blocks = [o for o in sc["ops"] if o[0] == "block"] + ops
    rest = [o for o in sc["ops"] if o[0] != "block"]
    dense = ("dense", [ID_POSE, ID_SPEEDBIAS, ID_POSE + 1, ID_SPEEDBIAS + 1], imu["residual"], imu["jacobians"], [1, 1, 0, 0])
    return dict(params={}, ops=blocks + [dense] + rest, rank=False)


SHARE = 128                      # LVI_MARG_SHARE: projection factors per partial


def gpu_scene(name):
    if name == "one_factor":                     # m = 7, n = 13
        return _projection_scene(1, [2], True, rank=True)
    if name in ("three_td", "three_plain"):      # 3 features over 4 frames, CauchyLoss(1), one 20-pixel outlier
        return _projection_scene(2, [4, 2, 3], name == "three_td", outlier=2, params=dict(tr_over_row=2e-5))
    if name == "share_plus_1":
        return _projection_scene(3, [3] * 65, True, count=SHARE + 1)
    if name == "two_partials_plus_1":
        return _projection_scene(4, [3] * 129, True, count=2 * SHARE + 1)
    if name == "eig_3_6":                        # m odd, n even, an untouched kept block
        return _dense_scene(5, [3], [2, 4], 8, zero_block=1)
    if name == "eig_7_12":                       # m = 6 + 1, n = 9 + 1 + 2
        return _dense_scene(6, [7, 1], [9, 1, 2], 30)
    if name == "eig_4_5":                        # m even, n odd, fewer rows than columns
        return _dense_scene(7, [2, 2], [3, 2], 6)
    if name == "eig_1_1":
        return _dense_scene(8, [1], [1], 3)
    if name == "eig_2_3":
        return _dense_scene(9, [2], [1, 2], 9)
    # the eigen-solver's one width: its 1024 threads stride over dim' / 2 pairs x dim entries of a round, one pass up to
    # dim = 44 (22 x 44 = 968), two from dim = 45 (23 x 45 = 1035)
    if name == "eig_44_45":                      # m the last size of one pass, n the first of two
        return _dense_scene(11, [9, 9, 9, 9, 8], [9, 9, 9, 9, 9], 120)
    if name == "eig_45_46":                      # both past it, m odd, n even
        return _dense_scene(12, [9, 9, 9, 9, 9], [9, 9, 9, 9, 9, 1], 120)
    if name == "imu_1e10":
        return _imu_scene(10, 1e10)
    raise KeyError(name)


GPU_SCENES = ["one_factor", "three_td", "three_plain", "share_plus_1", "two_partials_plus_1", "eig_3_6", "eig_7_12", "eig_4_5", "eig_1_1", "eig_2_3", "eig_44_45", "eig_45_46", "imu_1e10"]
SYSTEM_ONLY = ("share_plus_1", "two_partials_plus_1")        # compared on A and b


def play(scene, M):
    """issue a scene's script on anything with set_block / add_projection / add_dense"""
    for op in scene["ops"]:
        if op[0] == "block":
            M.set_block(op[1], op[2])
        elif op[0] == "proj":
            M.add_projection(op[1])
        else:
            M.add_dense(*op[1:])
    return M


_cache = {}


def scene_reference(name):
    """-> (float64 result, mpmath result) of a scene, computed once; a SYSTEM_ONLY scene has A, b, m, n only"""
    if name not in _cache:
        sc, out = gpu_scene(name), []
        for X in (F64, MP):
            M = play(sc, Marg(X, **sc["params"]))
            if name in SYSTEM_ONLY:
                A, b, m, n = M.system()
                out.append(dict(A=A, b=b, m=m, n=n))
            else:
                out.append(M.marginalize())
        _cache[name] = tuple(out)
    return _cache[name]


# the chain of the GPU tier: MARGIN_OLD -> MARGIN_SECOND_NEW -> MARGIN_OLD with changed values between
CHAIN_FEATURES, CHAIN_INFO = 8, 1e4


def chain_steps():
    """-> [(flag, window, features, imu)]: the inputs of the three steps.  The second and third windows are the slid ones
    with perturbed values, pose 3 and the extrinsic's quaternion with flipped signs in the third."""
    win0, feats0 = make_window(20, CHAIN_FEATURES, frames_seen=[11, 3, 2, 5], first_frames=(0, 0, 0, 2))
    win1 = perturb_window(shift_window(win0, MARGIN_OLD, 21), 22)
    win2 = perturb_window(shift_window(win1, MARGIN_SECOND_NEW, 23), 24, flip=(3,))
    win2["ex"][3:] *= -1
    _, feats2 = make_window(25, CHAIN_FEATURES, frames_seen=[4, 11, 2], first_frames=(0, 1, 0))
    return [(MARGIN_OLD, win0, feats0, imu_block(26, CHAIN_INFO)), (MARGIN_SECOND_NEW, win1, [], None), (MARGIN_OLD, win2, feats2, imu_block(27, CHAIN_INFO))]


def chain_reference():
    """-> per step (float64 prior, mpmath prior)"""
    if "chain" not in _cache:
        out, pf, pm = [], None, None
        for flag, win, feats, imu in chain_steps():
            pf = vins_marginalize(F64, pf, flag, win, feats, imu)
            pm = vins_marginalize(MP, pm, flag, win, feats, imu)
            out.append((pf, pm))
        _cache["chain"] = out
    return _cache["chain"]
