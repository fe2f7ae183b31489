"""float64 numpy reference of the pose-graph optimiser (include/lvi_pgo.h): the cost of mapOptimization.cpp's
factor graph without GPS (the prior of :1418-1420, the odometry BetweenFactors of :1422-1427, the loop BetweenFactors of
:1509-1527) and its minimiser by undamped Gauss-Newton on SE(3).

The conventions restate GTSAM's Pose3 (recalled; GTSAM is not vendored): tangent = (rotation, translation), right
perturbations X <- X Retract(delta), error = Local(measured^-1 h(x)) whitened by 1 / sqrt(variance), and the chart switch
``full_logmap``: 1 = Pose3::Logmap / Expmap, 0 = [Rot3::Logmap(R); t] / (Rot3::Expmap(w), v).  The formulas and the series
switches are those of csrc/lvi_pgo_math.hpp; the analytic Jacobians are checked against central differences in
tests/test_pgo_ref.py.

Every Gauss-Newton step can be computed by two independent linear solves:
  "chol"   Cholesky of the normal equations J'J delta = -J'r (dense; above DENSE_N poses SuperLU without pivoting in the
           natural order, which on an SPD matrix is its LDL' factorisation)
  "lstsq"  least squares on the whitened Jacobian itself (dense LAPACK gelsd; above DENSE_N poses the sparse augmented
           system [[I, J], [J', 0]] by SuperLU with partial pivoting), which never forms J'J
``solve_both`` runs the whole iteration once with each and returns both answers; their distance is the yardstick G of
the GPU tier.

The gauge.  Every between factor is invariant under a common left transform of all poses, so J_between N = 0 for the six
gauge directions N (node i's block: Ad(X_i^-1)) at ANY linearisation point, and the prior is the only factor that sees
them.  Projecting the normal equations on N leaves B_prior delta_0 = -r_prior exactly: the step of node 0 is fixed by the
prior alone, whatever its covariance, and the other nodes follow from the between factors with delta_0 substituted.
gauge="anchored" (the default) computes the step this way; gauge="full" solves the system as it stands.  In exact
arithmetic the two are the same step.  In double they are not: the translation prior's information is 1e-8 beside 1e6
of the odometry, the rounding of J'r (about 1e-13) divided by 1e-8 is a random common translation of 1e-8 .. 1e-5 per
step, and NEITHER linear solver on the full system ever reaches max|delta| < 1e-10 (measured in test_pgo_ref.py; the
poses relative to X0 agree with the anchored answer to 1e-12 all the same).  The device solver is anchored."""
import numpy as np

F32, F64 = np.float32, np.float64
SERIES_TH2 = 0.04
PRIOR_VAR = np.array([1e-2, 1e-2, np.pi * np.pi, 1e8, 1e8, 1e8])        # mapOptimization.cpp:1418-1420
ODOM_VAR = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])              # :1424
CONV_EPS, MAX_ITERS = 1e-10, 10
DENSE_N = 64


# ---- SO(3) / SE(3) ---------------------------------------------------------------------------------
def so3_abc(th2):
    if th2 < SERIES_TH2:
        a = 1. - th2 / 6. * (1. - th2 / 20. * (1. - th2 / 42. * (1. - th2 / 72. * (1. - th2 / 110.))))
        b = .5 - th2 / 24. * (1. - th2 / 30. * (1. - th2 / 56. * (1. - th2 / 90. * (1. - th2 / 132.))))
        c = 1. / 6. - th2 / 120. * (1. - th2 / 42. * (1. - th2 / 72. * (1. - th2 / 110. * (1. - th2 / 156.))))
        return a, b, c
    th = np.sqrt(th2)
    s, co = np.sin(th), np.cos(th)
    return s / th, (1. - co) / th2, (th - s) / (th2 * th)


def so3_g(th2):
    if th2 < SERIES_TH2:
        return 1. / 12. + th2 * (1. / 720. + th2 * (1. / 30240. + th2 * (1. / 1209600. + th2 * (1. / 47900160. + th2 * (691. / 1307674368000.)))))
    a, b, _ = so3_abc(th2)
    return (1. - a / (2. * b)) / th2


def se3_de(th2):
    if th2 < SERIES_TH2:
        d = 1. / 24. - th2 / 720. * (1. - th2 / 56. * (1. - th2 / 90. * (1. - th2 / 132. * (1. - th2 / 182.))))
        e = 1. / 120. + th2 * (-2. / 5040. + th2 * (3. / 362880. + th2 * (-4. / 39916800. + th2 * (5. / 6227020800. + th2 * (-6. / 1307674368000.)))))
        return d, e
    th = np.sqrt(th2)
    s, co = np.sin(th), np.cos(th)
    return (th2 + 2. * co - 2.) / (2. * th2 * th2), (2. * th - 3. * s + th * co) / (2. * th2 * th2 * th)


def hat(w):
    return np.array([[0., -w[2], w[1]], [w[2], 0., -w[0]], [-w[1], w[0], 0.]])


def poly_w(w, s0, s1, s2):
    W = hat(w)
    return s0 * np.eye(3) + s1 * W + s2 * (W @ W)


def so3_exp(w):
    a, b, _ = so3_abc(float(np.dot(w, w)))
    return poly_w(w, 1., a, b)


def so3_log(R):
    v = .5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, co = float(np.sqrt(np.dot(v, v))), .5 * (np.trace(R) - 1.)
    th = float(np.arctan2(s, co))
    if co > -0.9:
        k = 1. / so3_abc(th * th)[0] if th * th < SERIES_TH2 else th / s
        return k * v
    k = int(np.argmax(np.diag(R)))
    ak = np.sqrt((R[k, k] - co) / (1. - co))
    ax = np.array([ak if j == k else .5 * (R[k, j] + R[j, k]) / ((1. - co) * ak) for j in range(3)])
    sg = -1. if float(np.dot(ax, v)) < 0. else 1.
    return sg * th * ax / np.sqrt(np.dot(ax, ax))


def so3_jr_inv(w):
    return poly_w(w, 1., .5, so3_g(float(np.dot(w, w))))


def pose_exp(xi, full=1):
    T = np.eye(4)
    T[:3, :3] = so3_exp(xi[:3])
    if full:
        _, b, c = so3_abc(float(np.dot(xi[:3], xi[:3])))
        T[:3, 3] = poly_w(xi[:3], 1., b, c) @ xi[3:]
    else:
        T[:3, 3] = xi[3:]
    return T


def pose_log(T, full=1):
    w = so3_log(T[:3, :3])
    u = poly_w(w, 1., -.5, so3_g(float(np.dot(w, w)))) @ T[:3, 3] if full else T[:3, 3]
    return np.r_[w, u]


def pose_inv(T):
    o = np.eye(4)
    o[:3, :3] = T[:3, :3].T
    o[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return o


def adjoint(T):
    R = T[:3, :3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, :3] = hat(T[:3, 3]) @ R
    A[3:, 3:] = R
    return A


def se3_q(phi, rho):
    th2 = float(np.dot(phi, phi))
    _, _, c = so3_abc(th2)
    d, e = se3_de(th2)
    P, R = hat(phi), hat(rho)
    PRP = P @ R @ P
    return .5 * R + c * (P @ R + R @ P + PRP) + d * (P @ P @ R + R @ P @ P - 3. * PRP) + e * (PRP @ P + P @ PRP)


def pose_local_jac(E, xi, full=1):
    Ji = so3_jr_inv(xi[:3])
    J = np.zeros((6, 6))
    J[:3, :3] = Ji
    if full:
        J[3:, :3] = -Ji @ se3_q(-xi[:3], -xi[3:]) @ Ji
        J[3:, 3:] = Ji
    else:
        J[3:, 3:] = E[:3, :3]
    return J


def prior_error(X, Z, full=1):
    E = pose_inv(Z) @ X
    r = pose_log(E, full)
    return r, pose_local_jac(E, r, full)


def between_error(Xi, Xj, Z, full=1):
    h = pose_inv(Xi) @ Xj
    E = pose_inv(Z) @ h
    r = pose_log(E, full)
    B = pose_local_jac(E, r, full)
    return r, -B @ adjoint(pose_inv(h)), B


def pose_from_rpyxyz(p):
    """Pose3(Rot3::RzRyRx(roll, pitch, yaw), Point3(x, y, z)) of a float pose, in double"""
    roll, pitch, yaw, x, y, z = [float(v) for v in np.asarray(p, F32)]
    A, B, C, D, E, F = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    return np.array([[A * C, A * D * F - B * E, B * F + A * D * E, x], [B * C, A * E + B * D * F, B * D * E - A * F, y], [-D, C * F, C * E, z], [0, 0, 0, 1.]])


def pose_to_rpyxyz(T):
    R = T[:3, :3]
    return np.array([np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], np.hypot(R[2, 1], R[2, 2])), np.arctan2(R[1, 0], R[0, 0]), *T[:3, 3]], F64).astype(F32)


def rot_angle(R):
    return float(np.sqrt(np.dot(so3_log(R), so3_log(R))))


def _solve_ls(J, r, solver, sparse):
    """argmin |J x + r| by the named linear solver"""
    if solver == "chol":
        if sparse:
            import scipy.sparse as sp
            import scipy.sparse.linalg as spl
            H = sp.csc_matrix(J.T @ J)
            lu = spl.splu(H, permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
            return lu.solve(-(J.T @ r))
        L = np.linalg.cholesky(J.T @ J)
        y = np.linalg.solve(L, -(J.T @ r))
        return np.linalg.solve(L.T, y)
    if solver == "lstsq":
        if sparse:
            import scipy.sparse as sp
            import scipy.sparse.linalg as spl
            m = J.shape[0]
            K = sp.bmat([[sp.identity(m, format="csc"), J], [J.T, None]], format="csc")
            return spl.splu(K).solve(np.r_[-r, np.zeros(J.shape[1])])[m:]
        return np.linalg.lstsq(J, -r, rcond=None)[0]
    raise ValueError(solver)


# ---- the graph ----------------------------------------------------------------------------------------
class Graph:
    """the calls of include/lvi_pgo.h on the host"""

    def __init__(self, full_logmap=1, conv_eps=CONV_EPS, max_iters=MAX_ITERS):
        self.full, self.eps, self.max_iters = int(full_logmap), float(conv_eps), int(max_iters)
        self.X, self.Zc, self.loops = [], [], []

    def copy(self):
        g = Graph(self.full, self.eps, self.max_iters)
        g.X, g.Zc, g.loops = [x.copy() for x in self.X], list(self.Zc), list(self.loops)
        return g

    def add_pose(self, pose_from, pose_to):
        to = pose_from_rpyxyz(pose_to)
        if not self.X:
            self.Zc.append(to)
        else:
            self.Zc.append(pose_inv(pose_from_rpyxyz(pose_from)) @ to)
        self.X.append(to)
        return len(self.X) - 1

    def add_loop(self, frm, to, between, variance):
        n = len(self.X)
        if frm == to or not (0 <= frm < n and 0 <= to < n) or not float(F32(variance)) > 0:
            raise ValueError("bad loop")
        self.loops.append((int(frm), int(to), np.array(between, F64).reshape(4, 4), float(F32(variance))))

    def edges(self):
        """(i, j, r, A, B, sqrt information [6]); i = -1 for the prior"""
        out = []
        sp, so = 1. / np.sqrt(PRIOR_VAR), 1. / np.sqrt(ODOM_VAR)
        for k in range(len(self.X)):
            if k == 0:
                r, B = prior_error(self.X[0], self.Zc[0], self.full)
                out.append((-1, 0, r, None, B, sp))
            else:
                r, A, B = between_error(self.X[k - 1], self.X[k], self.Zc[k], self.full)
                out.append((k - 1, k, r, A, B, so))
        for frm, to, Z, var in self.loops:
            r, A, B = between_error(self.X[frm], self.X[to], Z, self.full)
            out.append((frm, to, r, A, B, np.full(6, 1. / np.sqrt(var))))
        return out

    def chi2(self):
        return float(sum(np.dot(s * r, s * r) for _, _, r, _, _, s in self.edges()))

    def linear_system(self, sparse):
        """the whitened Jacobian J [6 E, 6 N] and residual r [6 E]"""
        ed = self.edges()
        n = len(self.X)
        rows, cols, vals = [], [], []
        r = np.zeros(6 * len(ed))
        for e, (i, j, re, A, B, s) in enumerate(ed):
            r[6 * e:6 * e + 6] = s * re
            for node, M in ((i, A), (j, B)):
                if M is None:
                    continue
                Mw = s[:, None] * M
                rr, cc = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
                rows.append((6 * e + rr).ravel()); cols.append((6 * node + cc).ravel()); vals.append(Mw.ravel())
        rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
        if sparse:
            import scipy.sparse as sp
            return sp.csc_matrix((vals, (rows, cols)), shape=(6 * len(ed), 6 * n)), r
        J = np.zeros((6 * len(ed), 6 * n))
        np.add.at(J, (rows, cols), vals)
        return J, r

    def step(self, solver, gauge="anchored"):
        """one Gauss-Newton step delta [6 N].  gauge = "full": the linear system as it stands.  gauge = "anchored": the same
        system with node 0 eliminated exactly (module docstring): delta_0 = -B_prior^-1 r_prior, the rest from the between
        factors alone with delta_0 substituted."""
        n = len(self.X)
        sparse = n > DENSE_N
        J, r = self.linear_system(sparse)
        if gauge == "full":
            return _solve_ls(J, r, solver, sparse)
        r0, B0 = prior_error(self.X[0], self.Zc[0], self.full)
        d0 = np.linalg.solve(B0, -r0)
        if n == 1:
            return d0
        Jr = J[6:, :]
        rr = r[6:] + Jr[:, :6] @ d0
        return np.r_[d0, _solve_ls(Jr[:, 6:], rr, solver, sparse)]

    def solve(self, solver="lstsq", gauge="anchored"):
        """undamped Gauss-Newton to max|delta| < conv_eps; -> dict(iterations, converged, chi2_before, chi2_after, max_step)"""
        info = dict(iterations=0, converged=False, chi2_before=self.chi2(), max_step=0.0, steps=[])
        for _ in range(self.max_iters):
            d = self.step(solver, gauge)
            for k in range(len(self.X)):
                self.X[k] = self.X[k] @ pose_exp(d[6 * k:6 * k + 6], self.full)
            info["iterations"] += 1
            info["max_step"] = float(np.abs(d).max())
            info["steps"].append(info["max_step"])
            if info["max_step"] < self.eps:
                info["converged"] = True
                break
        info["chi2_after"] = self.chi2()
        return info

    def poses(self):
        return np.array(self.X)


def solve_both(g, gauge="anchored"):
    """the graph solved once with each linear solver -> ((poses, info) of lstsq, (poses, info) of chol); g itself takes the lstsq answer"""
    gc = g.copy()
    ia = g.solve("lstsq", gauge)
    ib = gc.solve("chol", gauge)
    return (g.poses(), ia), (gc.poses(), ib)


def gaps(Xa, Xb):
    """(rotation angle, translation) of the largest difference between X0^-1 Xi of the two sets, and the same of X0"""
    ra = ta = 0.0
    A0, B0 = pose_inv(Xa[0]), pose_inv(Xb[0])
    for a, b in zip(Xa[1:], Xb[1:]):
        D = pose_inv(A0 @ a) @ (B0 @ b)
        ra, ta = max(ra, rot_angle(D[:3, :3])), max(ta, float(np.linalg.norm(D[:3, 3])))
    D0 = pose_inv(Xa[0]) @ Xb[0]
    return (ra, ta), (rot_angle(D0[:3, :3]), float(np.linalg.norm(D0[:3, 3])))


# ---- scenes ---------------------------------------------------------------------------------------------
def trajectory(n, seed, turns=1.0, radius=None, yaw0=0.0):
    """ground truth: a closed planar-ish circuit with roll / pitch / height wiggle, `turns` times round"""
    rs = np.random.RandomState(seed)
    radius = radius if radius is not None else max(2.0, 0.5 * n / (2 * np.pi * turns))      # about 0.5 m between keys
    ph = rs.uniform(0, 2 * np.pi, 3)
    out = []
    for k in range(n):
        a = 2 * np.pi * turns * k / max(n - 1, 1)
        yaw = yaw0 + a + np.pi / 2
        yaw = (yaw + np.pi) % (2 * np.pi) - np.pi
        T = pose_from_rpyxyz(F32([0.05 * np.sin(3 * a + ph[0]), 0.04 * np.sin(2 * a + ph[1]), yaw, radius * np.cos(a), radius * np.sin(a), 0.3 * np.sin(a + ph[2])]))
        out.append(T)
    return out


def scene(n, loops, seed, turns=1.0, yaw0=0.0, drift=1.0):
    """-> dict(poses f32 [n, 6] (the odometry chain, what the node would push), loops [(from, to, between 4x4, variance)], gt)
    Odometry noise is sized so that the accumulated drift stays below about 0.5 m and 5 degrees over the chain."""
    rs = np.random.RandomState(seed + 1000)
    gt = trajectory(n, seed, turns, yaw0=yaw0)
    radius = max(2.0, 0.5 * n / (2 * np.pi * turns))
    st, sr = drift * 0.1 / np.sqrt(max(n, 2)), drift * 0.15 / (max(radius, 4.0) * np.sqrt(max(n, 2)))
    X = [gt[0]]
    for k in range(1, n):
        noise = np.r_[rs.normal(0, sr, 3), rs.normal(0, st, 3)]
        X.append(X[-1] @ pose_inv(gt[k - 1]) @ gt[k] @ pose_exp(noise))
    poses = np.array([pose_to_rpyxyz(T) for T in X], F32)
    lp = []
    for frm, to in loops:
        noise = np.r_[rs.normal(0, 0.002, 3), rs.normal(0, 0.01, 3)]
        lp.append((frm, to, pose_inv(gt[frm]) @ gt[to] @ pose_exp(noise), float(F32(rs.uniform(0.05, 0.3)))))
    return dict(poses=poses, loops=lp, gt=gt)


def build(sc, g):
    """feed a scene to a Graph-like object (add_pose / add_loop)"""
    p = sc["poses"]
    for k in range(len(p)):
        g.add_pose(None if k == 0 else p[k - 1], p[k])
    for frm, to, Z, var in sc["loops"]:
        g.add_loop(frm, to, Z, var)
    return g


# the GPU tier's scenes: name -> (n, loops (from, to), seed, keyword arguments of scene)
GPU_SCENES = {
    "n1": (1, [], 1, {}),
    "n2": (2, [], 2, {}),
    "n3_loop": (3, [(2, 0)], 3, {}),
    # two loops share node 36, one joins neighbours i+1 -> i, one has from < to
    "n37": (37, [(36, 0), (2, 36), (20, 19)], 4, {}),
    "n300": (300, [(299, 0), (290, 5), (280, 12), (150, 149), (10, 270)], 5, {}),
    "n1025": (1025, [(1024, 0), (1000, 10), (990, 30), (512, 2), (700, 690), (20, 1010), (1024, 40), (800, 100)], 6, {}),
    # the heading starts near +pi and wraps through -pi on the way round
    "yaw_pi": (48, [(47, 0), (40, 3)], 7, dict(yaw0=np.pi / 2 - 0.3)),
}


def gpu_scene(name):
    n, loops, seed, kw = GPU_SCENES[name]
    return scene(n, loops, seed, **kw)
