"""Reference of the sliding-window solve (include/lvi_win.h): a restatement of IMUFactor::Evaluate
(imu_factor.h:18-178), IntegrationBase::evaluate (integration_base.h:160-186), MarginalizationFactor::Evaluate
(marginalization_factor.cpp:332-380), PoseLocalParameterization::Plus (pose_local_parameterization.cpp:3-19), the problem
build of estimator.cpp:696-789 and the trust-region loop with a traditional dogleg step that DESIGN §22 states, in two
arithmetics from the same float64 inputs: numpy float64 (`F64`) and mpmath at 50 digits (`MP`).  The projection factors
and the loss correction are tests/marg_ref.py's.  Scene preintegrations come from a numpy restatement of
midPointIntegration and propagate (integration_base.h:54-158): test infrastructure only.  Every decision of the loop is
reported with its margin.  Nothing here reads the library."""
import math

import numpy as np

import marg_ref as M
from marg_ref import F64, MP, local_size  # noqa: F401

CONSTANT, ELIMINATED = 1, 2
TERM_NONE, TERM_FUNCTION, TERM_GRADIENT, TERM_PARAMETER, TERM_ITERATIONS, TERM_TIME, TERM_RADIUS, TERM_INVALID_STEPS = range(8)
STEP_NONE, STEP_GAUSS_NEWTON, STEP_CAUCHY, STEP_INTERPOLATED = range(4)
O_P, O_R, O_V, O_BA, O_BG = 0, 3, 6, 9, 12
SHARE, CHOL_BLOCK = 128, 32

# the loop's constants; the ones marked R in include/lvi_win.h are restated from recall of ceres-solver's defaults
DEFAULTS = dict(loss_type=M.LOSS_CAUCHY, max_iterations=8, jacobi_scaling=1, max_invalid_steps=5, loss_a=1.0, sqrt_info=M.SQRT_INFO, tr_over_row=0.0,
                half_row=240.0, G=(0.0, 0.0, 9.8), max_time_s=0.0, initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3,
                function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8, initial_mu=1e-8, min_mu=1e-8, max_mu=1.0,
                mu_increase_factor=10.0, increase_threshold=0.75, decrease_threshold=0.25, min_diagonal=1e-6, max_diagonal=1e32)


# ---- quaternions (x y z w) ----------------------------------------------------------------------------------
def qmul(a, b, X):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]], X.dtype)


def qinv(q, X):
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return np.array([-q[0] / n2, -q[1] / n2, -q[2] / n2, q[3] / n2], X.dtype)


def delta_q(theta, X):
    """Utility::deltaQ: (1, theta / 2), not normalised"""
    two = X.num(2.0)
    return np.array([theta[0] / two, theta[1] / two, theta[2] / two, X.num(1.0)], X.dtype)


def qleft_br(q, X):
    """bottomRightCorner<3, 3>() of Utility::Qleft"""
    return q[3] * X.arr(np.eye(3)) + M.skew(q[:3], X)


def qleft_qright_br(a, b, X):
    """... of Qleft(a) * Qright(b)"""
    L = qleft_br(a, X)
    R = b[3] * X.arr(np.eye(3)) - M.skew(b[:3], X)
    return L @ R - np.outer(a[:3], b[:3])


def pose_plus(x, d, X):
    q = qmul(x[3:7], delta_q(d[3:6], X), X)
    n = X.sqrt(sum(v * v for v in q))
    return np.concatenate([x[:3] + d[:3], q / n])


# ---- sqrt_info ----------------------------------------------------------------------------------------------
def chol_lower(A, X):
    """-> (L, pivots): the lower Cholesky factor; None when a pivot is not positive"""
    n = A.shape[0]
    L, piv = X.zeros(n, n), []
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        piv.append(d)
        if not d > 0:
            return None, piv
        s = X.sqrt(d)
        L[j, j] = s
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / s
    return L, piv


def imu_sqrt_info(cov, X):
    """imu_factor.h:63: covariance = C C', covariance^-1 = C^-T C^-1, its LLT factor L, sqrt_info = L'"""
    n = 15
    C, _ = chol_lower(X.arr(cov), X)
    Ci, one = X.zeros(n, n), X.num(1.0)
    for j in range(n):
        Ci[j, j] = one / C[j, j]
        for i in range(j + 1, n):
            Ci[i, j] = -sum(C[i, k] * Ci[k, j] for k in range(j, i)) / C[i, i]
    L, _ = chol_lower(Ci.T @ Ci, X)
    return L.T


# ---- IMUFactor ---------------------------------------------------------------------------------------------
def imu_eval_raw(pose_i, sb_i, pose_j, sb_j, pre, G, X, jac=True):
    """-> (r [15], J [15, 30] or None) before sqrt_info; columns pose_i 0..5, speed_bias_i 6..14, pose_j 15..20, speed_bias_j 21..29"""
    A = X.arr
    pose_i, sb_i, pose_j, sb_j, G = A(pose_i), A(sb_i), A(pose_j), A(sb_j), A(G)
    Pi, Qi, Vi, Bai, Bgi = pose_i[:3], pose_i[3:7], sb_i[:3], sb_i[3:6], sb_i[6:9]
    Pj, Qj, Vj, Baj, Bgj = pose_j[:3], pose_j[3:7], sb_j[:3], sb_j[3:6], sb_j[6:9]
    dt, jm = X.num(pre["sum_dt"]), A(pre["jacobian"])
    dp_dba, dp_dbg, dq_dbg = jm[O_P:O_P + 3, O_BA:O_BA + 3], jm[O_P:O_P + 3, O_BG:O_BG + 3], jm[O_R:O_R + 3, O_BG:O_BG + 3]
    dv_dba, dv_dbg = jm[O_V:O_V + 3, O_BA:O_BA + 3], jm[O_V:O_V + 3, O_BG:O_BG + 3]
    dba, dbg = Bai - A(pre["linearized_ba"]), Bgi - A(pre["linearized_bg"])
    dq0 = A(pre["delta_q"])
    cdq = qmul(dq0, delta_q(dq_dbg @ dbg, X), X)
    cdv = A(pre["delta_v"]) + dv_dba @ dba + dv_dbg @ dbg
    cdp = A(pre["delta_p"]) + dp_dba @ dba + dp_dbg @ dbg
    Ri = M.quat_to_rot(Qi, X)
    half, two = X.num(0.5), X.num(2.0)
    rp = Ri.T @ (half * G * dt * dt + Pj - Pi - Vi * dt)
    rv = Ri.T @ (G * dt + Vj - Vi)
    QiQj = qmul(qinv(Qi, X), Qj, X)
    cdq_inv = qinv(cdq, X)
    r = np.concatenate([rp - cdp, two * qmul(cdq_inv, QiQj, X)[:3], rv - cdv, Baj - Bai, Bgj - Bgi])
    if not jac:
        return r, None
    J, eye = X.zeros(15, 30), A(np.eye(3))
    QjQi = qmul(qinv(Qj, X), Qi, X)
    J[O_P:O_P + 3, 0:3] = -Ri.T
    J[O_P:O_P + 3, 3:6] = M.skew(rp, X)
    J[O_R:O_R + 3, 3:6] = -qleft_qright_br(QjQi, cdq, X)
    J[O_V:O_V + 3, 3:6] = M.skew(rv, X)
    J[O_P:O_P + 3, 6:9] = -Ri.T * dt
    J[O_P:O_P + 3, 9:12] = -dp_dba
    J[O_P:O_P + 3, 12:15] = -dp_dbg
    J[O_R:O_R + 3, 12:15] = -qleft_br(qmul(QjQi, dq0, X), X) @ dq_dbg
    J[O_V:O_V + 3, 6:9] = -Ri.T
    J[O_V:O_V + 3, 9:12] = -dv_dba
    J[O_V:O_V + 3, 12:15] = -dv_dbg
    J[O_BA:O_BA + 3, 9:12] = -eye
    J[O_BG:O_BG + 3, 12:15] = -eye
    J[O_P:O_P + 3, 15:18] = Ri.T
    J[O_R:O_R + 3, 18:21] = qleft_br(qmul(cdq_inv, QiQj, X), X)
    J[O_V:O_V + 3, 21:24] = Ri.T
    J[O_BA:O_BA + 3, 24:27] = eye
    J[O_BG:O_BG + 3, 27:30] = eye
    return r, J


def imu_factor(pose_i, sb_i, pose_j, sb_j, pre, G, X, sqrt_info=None, jac=True):
    S = imu_sqrt_info(pre["covariance"], X) if sqrt_info is None else sqrt_info
    r, J = imu_eval_raw(pose_i, sb_i, pose_j, sb_j, pre, G, X, jac)
    return S @ r, (S @ J if jac else None)


def preintegrate(dts, accs, gyrs, ba, bg, acc_n=0.08, gyr_n=0.004, acc_w=0.00004, gyr_w=2.0e-6):
    """IntegrationBase over the samples (the first one initialises acc_0, gyr_0): float64 -> the fields of lvi_win_imu"""
    noise = np.diag(np.r_[[acc_n ** 2] * 3, [gyr_n ** 2] * 3, [acc_n ** 2] * 3, [gyr_n ** 2] * 3, [acc_w ** 2] * 3, [gyr_w ** 2] * 3])
    acc_0, gyr_0 = np.asarray(accs[0], float), np.asarray(gyrs[0], float)
    dp, dq, dv, Jm, cov, sum_dt = np.zeros(3), np.r_[0., 0., 0., 1.], np.zeros(3), np.eye(15), np.zeros((15, 15)), 0.0
    sk = lambda v: M.skew(v, F64)
    for dt, acc_1, gyr_1 in zip(dts[1:], accs[1:], gyrs[1:]):
        acc_1, gyr_1 = np.asarray(acc_1, float), np.asarray(gyr_1, float)
        R0 = M.rot(dq)
        un_acc_0 = R0 @ (acc_0 - ba)
        un_gyr = 0.5 * (gyr_0 + gyr_1) - bg
        rq = M.quat_mul(dq, np.r_[un_gyr * dt / 2, 1.0])
        R1 = _rot_unnormalised(rq)
        un_acc = 0.5 * (un_acc_0 + R1 @ (acc_1 - ba))
        rp, rvv = dp + dv * dt + 0.5 * un_acc * dt * dt, dv + un_acc * dt
        Rw, Ra0, Ra1, I3 = sk(un_gyr), sk(acc_0 - ba), sk(acc_1 - ba), np.eye(3)
        F = np.zeros((15, 15))
        F[0:3, 0:3] = I3
        F[0:3, 3:6] = -0.25 * R0 @ Ra0 * dt * dt + -0.25 * R1 @ Ra1 @ (I3 - Rw * dt) * dt * dt
        F[0:3, 6:9] = I3 * dt
        F[0:3, 9:12] = -0.25 * (R0 + R1) * dt * dt
        F[0:3, 12:15] = -0.25 * R1 @ Ra1 * dt * dt * -dt
        F[3:6, 3:6] = I3 - Rw * dt
        F[3:6, 12:15] = -1.0 * I3 * dt
        F[6:9, 3:6] = -0.5 * R0 @ Ra0 * dt + -0.5 * R1 @ Ra1 @ (I3 - Rw * dt) * dt
        F[6:9, 6:9] = I3
        F[6:9, 9:12] = -0.5 * (R0 + R1) * dt
        F[6:9, 12:15] = -0.5 * R1 @ Ra1 * dt * -dt
        F[9:12, 9:12] = I3
        F[12:15, 12:15] = I3
        V = np.zeros((15, 18))
        V[0:3, 0:3] = 0.25 * R0 * dt * dt
        V[0:3, 3:6] = 0.25 * -R1 @ Ra1 * dt * dt * 0.5 * dt
        V[0:3, 6:9] = 0.25 * R1 * dt * dt
        V[0:3, 9:12] = V[0:3, 3:6]
        V[3:6, 3:6] = 0.5 * I3 * dt
        V[3:6, 9:12] = 0.5 * I3 * dt
        V[6:9, 0:3] = 0.5 * R0 * dt
        V[6:9, 3:6] = 0.5 * -R1 @ Ra1 * dt * 0.5 * dt
        V[6:9, 6:9] = 0.5 * R1 * dt
        V[6:9, 9:12] = V[6:9, 3:6]
        V[9:12, 12:15] = I3 * dt
        V[12:15, 15:18] = I3 * dt
        Jm = F @ Jm
        cov = F @ cov @ F.T + V @ noise @ V.T
        dp, dv, dq = rp, rvv, rq / np.linalg.norm(rq)
        sum_dt += dt
        acc_0, gyr_0 = acc_1, gyr_1
    cov = 0.5 * (cov + cov.T)
    return dict(sum_dt=sum_dt, delta_p=dp, delta_q=dq, delta_v=dv, linearized_ba=np.asarray(ba, float), linearized_bg=np.asarray(bg, float), jacobian=Jm,
                covariance=cov)


def _rot_unnormalised(q):
    """Eigen's toRotationMatrix of a quaternion as it stands (result_delta_q is normalised only after the step)"""
    return M.quat_to_rot(np.asarray(q, np.float64), F64)


# ---- the problem ---------------------------------------------------------------------------------------------
class Problem:
    """estimator.cpp:696-789 in arithmetic X: blocks by id in order of declaration, projection records (dicts as
    tests/marg_ref.py's), IMU records (dicts with the block ids and the fields of `preintegrate`), a prior (the dict
    tests/marg_ref.py's marginalize returns, or its float64 arrays)"""

    def __init__(self, X, **params):
        self.X, self.P = X, dict(DEFAULTS)
        self.P.update(params)
        self.order, self.values, self.flags = [], {}, {}
        self.proj, self.imu, self.prior, self._sinfo = [], [], None, {}

    def set_block(self, bid, values, flags=0):
        if bid not in self.values:
            self.order.append(bid)
        self.values[bid], self.flags[bid] = np.array(values, np.float64), flags

    def add_projection(self, rec):
        self.proj.append(rec)

    def add_imu(self, rec):
        self.imu.append(rec)

    def set_prior(self, prior):
        X = self.X
        self.prior = dict(J=X.arr(M.to_f64(prior["J"])), r=X.arr(M.to_f64(prior["r"])), ids=list(prior["ids"]), sizes=list(prior["sizes"]),
                          col=list(prior["col"]), x0=[np.asarray(v, np.float64) for v in prior["x0"]])

    def layout(self):
        col, elim, D, E = {}, {}, 0, 0
        for b in self.order:
            if self.flags[b] & CONSTANT:
                continue
            if self.flags[b] & ELIMINATED:
                elim[b] = E
                E += 1
            else:
                col[b] = D
                D += local_size(len(self.values[b]))
        return col, elim, D, E

    def x0(self):
        return {b: self.X.arr(self.values[b]) for b in self.order}

    def factors(self, x, jac=True):
        """-> [(ids, r, [J per block] or None, cost)] in the order projections, IMU factors, prior"""
        X, P, out = self.X, self.P, []
        const = dict(sqrt_info=P["sqrt_info"], tr_over_row=P["tr_over_row"], half_row=P["half_row"])
        half = X.num(0.5)
        for rec in self.proj:
            use_td = rec["td"] != -1
            ids = [rec["pose_i"], rec["pose_j"], rec["ex"], rec["feature"]] + ([rec["td"]] if use_td else [])
            td = x[rec["td"]][0] if use_td else 0.0
            r, J = M.projection_eval(x[ids[0]], x[ids[1]], x[ids[2]], x[ids[3]][0], td, use_td, rec, X, **const)
            rho = M.loss_rho(P["loss_type"], P["loss_a"], sum(v * v for v in r), X)
            if P["loss_type"] != M.LOSS_NONE:
                r, J = M.loss_correct(r, J, rho, X)
            Js = [J[:, 0:6], J[:, 6:12], J[:, 12:18], J[:, 18:19]] + ([J[:, 19:20]] if use_td else [])
            out.append((ids, r, Js if jac else None, half * rho[0]))
        for k, rec in enumerate(self.imu):
            if k not in self._sinfo:
                self._sinfo[k] = imu_sqrt_info(rec["covariance"], X)
            ids = [rec["pose_i"], rec["speed_bias_i"], rec["pose_j"], rec["speed_bias_j"]]
            r, J = imu_factor(x[ids[0]], x[ids[1]], x[ids[2]], x[ids[3]], rec, P["G"], X, self._sinfo[k], jac)
            out.append((ids, r, [J[:, 0:6], J[:, 6:15], J[:, 15:21], J[:, 21:30]] if jac else None, half * sum(v * v for v in r)))
        if self.prior is not None:
            pr = self.prior
            dx = X.zeros(len(pr["r"]))
            for bid, size, c, v0 in zip(pr["ids"], pr["sizes"], pr["col"], pr["x0"]):
                dx[c:c + local_size(size)] = M.prior_dx(size, x[bid], v0, X)
            r = pr["r"] + pr["J"] @ dx
            Js = [pr["J"][:, c:c + local_size(s)] for c, s in zip(pr["col"], pr["sizes"])]
            out.append((list(pr["ids"]), r, Js if jac else None, half * sum(v * v for v in r)))
        return out

    def cost(self, x):
        return sum(f[3] for f in self.factors(x, jac=False))

    def system(self, x):
        """-> dict(H [D, D], g [D], W [E, D], h [E], gf [E], cost, rr, rows) before scaling: the camera side, the coupling and the
        eliminated diagonal; rr: the squared norm of all (loss-corrected) residuals, rows: their number"""
        X = self.X
        col, elim, D, E = self.layout()
        H, g, W, h, gf, cost, rr, rows = X.zeros(D, D), X.zeros(D), X.zeros(E, D), X.zeros(E), X.zeros(E), X.num(0.0), X.num(0.0), 0
        for ids, r, Js, c in self.factors(x):
            cost, rr, rows = cost + c, rr + r @ r, rows + len(r)
            cam = [(col[b], J) for b, J in zip(ids, Js) if b in col]
            for ci, Ji in cam:
                for cj, Jj in cam:
                    H[ci:ci + Ji.shape[1], cj:cj + Jj.shape[1]] += Ji.T @ Jj
                g[ci:ci + Ji.shape[1]] += Ji.T @ r
            for b, Jf in zip(ids, Js):
                if b in elim:
                    k, jf = elim[b], Jf[:, 0]
                    h[k] += jf @ jf
                    gf[k] += jf @ r
                    for ci, Ji in cam:
                        W[k, ci:ci + Ji.shape[1]] += jf @ Ji
        return dict(H=H, g=g, W=W, h=h, gf=gf, cost=cost, D=D, E=E, rr=rr, rows=rows)

    def plus(self, x, dc, df):
        X = self.X
        col, elim, _, _ = self.layout()
        out = {}
        for b in self.order:
            v = x[b]
            if b in col and len(v) == 7:
                out[b] = pose_plus(v, dc[col[b]:col[b] + 6], X)
            elif b in col:
                out[b] = v + dc[col[b]:col[b] + len(v)]
            elif b in elim:
                out[b] = v + df[elim[b]:elim[b] + 1]
            else:
                out[b] = v
        return out

    def x_norm(self, x):
        return self.X.sqrt(sum(v * v for b in self.order if not self.flags[b] & CONSTANT for v in x[b]))


def _clamp(v, lo, hi, X):
    return min(max(v, X.num(lo)), X.num(hi))


class Strategy:
    """the quantities of one linearisation: Jacobi scales (kept from the first one), the diagonal, the scaled gradient, alpha"""

    def __init__(self, prob, sys, scale=None):
        X, P = prob.X, prob.P
        self.X, self.P, self.sys = X, P, sys
        one = X.num(1.0)
        if scale is None:
            if P["jacobi_scaling"]:
                scale = (np.array([one / (one + X.sqrt(sys["H"][i, i])) for i in range(sys["D"])], X.dtype),
                         np.array([one / (one + X.sqrt(v)) for v in sys["h"]], X.dtype))
            else:
                scale = (np.array([one] * sys["D"], X.dtype), np.array([one] * sys["E"], X.dtype))
        self.sc, self.sf = scale
        sc, sf, H, h = self.sc, self.sf, sys["H"], sys["h"]
        self.dgc = np.array([X.sqrt(_clamp(sc[i] * H[i, i] * sc[i], P["min_diagonal"], P["max_diagonal"], X)) for i in range(sys["D"])], X.dtype)
        self.dgf = np.array([X.sqrt(_clamp(sf[k] * h[k] * sf[k], P["min_diagonal"], P["max_diagonal"], X)) for k in range(sys["E"])], X.dtype)
        self.grc, self.grf = sc * sys["g"] / self.dgc, sf * sys["gf"] / self.dgf
        self.grad_max = max([abs(v) for v in sys["g"]] + [abs(v) for v in sys["gf"]])
        gn2 = sum(v * v for v in self.grc) + sum(v * v for v in self.grf)
        self.grad_norm = X.sqrt(gn2)
        uc, uf = self.grc / self.dgc * sc, self.grf / self.dgf * sf
        self.alpha = gn2 / self.quad(uc, uf)

    def quad(self, uc, uf):
        s = self.sys
        return uc @ s["H"] @ uc + sum(self.X.num(2.0) * uf[k] * (s["W"][k] @ uc) + s["h"][k] * uf[k] * uf[k] for k in range(s["E"]))

    def reduced(self, mu):
        """-> (S [D, D], b [D], den [E]): the scaled, regularised Schur complement, its right-hand side, hs + mu dg^2"""
        X, s, sc, sf = self.X, self.sys, self.sc, self.sf
        mu = X.num(mu)
        S = sc[:, None] * s["H"] * sc[None, :]
        b = sc * s["g"]
        for i in range(s["D"]):
            S[i, i] = S[i, i] + mu * (self.dgc[i] * self.dgc[i])
        den = np.array([sf[k] * s["h"][k] * sf[k] + mu * (self.dgf[k] * self.dgf[k]) for k in range(s["E"])], X.dtype)
        for k in range(s["E"]):
            ws = sf[k] * s["W"][k] * sc
            S = S - np.outer(ws, ws) / den[k]
            b = b - ws * (sf[k] * s["gf"][k]) / den[k]
        return S, b, den

    def gauss_newton(self, mu):
        """-> (yc, yf, pivots) or (None, None, pivots) when a pivot is not positive"""
        X, s, sc, sf = self.X, self.sys, self.sc, self.sf
        S, b, den = self.reduced(mu)
        L, piv = chol_lower(S, X)
        if L is None:
            return None, None, piv
        D = s["D"]
        z = X.zeros(D)
        for i in range(D):
            z[i] = (b[i] - L[i, :i] @ z[:i]) / L[i, i]
        y = X.zeros(D)
        for i in reversed(range(D)):
            y[i] = (z[i] - L[i + 1:, i] @ y[i + 1:]) / L[i, i]
        yc = -y
        yf = np.array([(-(sf[k] * s["gf"][k]) - (sf[k] * s["W"][k] * sc) @ yc) / den[k] for k in range(s["E"])], X.dtype)
        return yc, yf, piv

    def dogleg(self, yc, yf, radius):
        """-> dict(kind, dc, df (tangent-space step, unscaled), gn_norm, cauchy_norm, dogleg_norm, model_cost_change, step_norm)"""
        X, s = self.X, self.sys
        radius = X.num(radius)
        dyc, dyf = self.dgc * yc, self.dgf * yf
        n2 = sum(v * v for v in dyc) + sum(v * v for v in dyf)
        dot = sum(a * b for a, b in zip(self.grc, dyc)) + sum(a * b for a, b in zip(self.grf, dyf))
        gn_norm, cauchy_norm = X.sqrt(n2), self.grad_norm * self.alpha
        one, two = X.num(1.0), X.num(2.0)
        if gn_norm <= radius:
            kind, stc, stf, dn = STEP_GAUSS_NEWTON, yc, yf, gn_norm
        elif cauchy_norm >= radius:
            ca = -(radius / self.grad_norm)
            kind, stc, stf, dn = STEP_CAUCHY, ca * self.grc / self.dgc, ca * self.grf / self.dgf, radius
        else:
            b_dot_a, a2 = -self.alpha * dot, cauchy_norm * cauchy_norm
            bma2 = a2 - two * b_dot_a + n2
            c = b_dot_a - a2
            dd = X.sqrt(c * c + bma2 * (radius * radius - a2))
            beta = (dd - c) / bma2 if c <= 0 else (radius * radius - a2) / (dd + c)
            ca = -self.alpha * (one - beta)
            kind, dn = STEP_INTERPOLATED, radius
            stc, stf = (ca * self.grc + beta * dyc) / self.dgc, (ca * self.grf + beta * dyf) / self.dgf
        dc, df = stc * self.sc, stf * self.sf
        gd = dc @ s["g"] + (df @ s["gf"] if s["E"] else X.num(0.0))
        mcc = -(gd + X.num(0.5) * self.quad(dc, df))
        return dict(kind=kind, dc=dc, df=df, gn_norm=gn_norm, cauchy_norm=cauchy_norm, dogleg_norm=dn, model_cost_change=mcc,
                    step_norm=X.sqrt(sum(v * v for v in dc) + sum(v * v for v in df)))


def solve(prob, x=None, radius=None, mu=None):
    """the trust-region loop of DESIGN §22 -> dict(x, log, iterates, termination, iterations, cost, initial_cost, radius, mu).
    A log entry holds the fields of lvi_win_iteration and `margins`: [(decision, value, threshold)] of everything the entry
    decided; `iterates` holds, per iteration, the state (x, radius, mu, reuse) it started from."""
    X, P = prob.X, prob.P
    x = prob.x0() if x is None else x
    radius = X.num(P["initial_radius"] if radius is None else radius)
    mu = X.num(P["initial_mu"] if mu is None else mu)
    sys = prob.system(x)
    st = Strategy(prob, sys)
    scale = (st.sc, st.sf)
    cost = sys["cost"]
    log = [dict(iteration=0, step_kind=0, accepted=0, mu_retries=0, cost=cost, gradient_max_norm=st.grad_max, radius=radius, mu=mu,
                margins=[("gradient_tolerance", st.grad_max, P["gradient_tolerance"])])]
    out = dict(initial_cost=cost, iterates=[])
    term = TERM_GRADIENT if st.grad_max <= P["gradient_tolerance"] else TERM_NONE
    it, invalid, reuse, gn = 0, 0, False, None
    while term == TERM_NONE:
        if it >= P["max_iterations"]:
            term = TERM_ITERATIONS
            break
        it += 1
        out["iterates"].append(dict(x=x, radius=radius, mu=mu, reuse=reuse))
        e = dict(iteration=it, step_kind=0, accepted=0, mu_retries=0, cost=cost, gradient_max_norm=st.grad_max, radius=radius, margins=[])
        ok = reuse
        if not reuse:
            gn = None
            while mu < P["max_mu"]:
                yc, yf, piv = st.gauss_newton(mu)
                e["margins"].append(("pivot", min(piv), 0.0))
                if yc is None:
                    mu = mu * X.num(P["mu_increase_factor"])
                    e["mu_retries"] += 1
                    continue
                gn, ok = (yc, yf), True
                break
        e["mu"] = mu
        if ok:
            d = st.dogleg(gn[0], gn[1], radius)
            e.update(step_kind=d["kind"], gauss_newton_norm=d["gn_norm"], cauchy_norm=d["cauchy_norm"], model_cost_change=d["model_cost_change"],
                     step_norm=d["step_norm"])
            e["margins"] += [("gn_norm_vs_radius", d["gn_norm"], radius), ("cauchy_norm_vs_radius", d["cauchy_norm"], radius),
                             ("model_cost_change", d["model_cost_change"], 0.0)]
        if not (ok and d["model_cost_change"] > 0):
            invalid += 1
            log.append(e)
            if invalid >= P["max_invalid_steps"]:
                term = TERM_INVALID_STEPS
                break
            radius, reuse = radius * X.num(0.5), ok
            if radius < P["min_radius"]:
                term = TERM_RADIUS
            continue
        invalid = 0
        cand = prob.plus(x, d["dc"], d["df"])
        cand_cost = prob.cost(cand)
        e["cost_change"] = cost - cand_cost
        e["rho"] = e["cost_change"] / d["model_cost_change"]
        ptol = X.num(P["parameter_tolerance"])
        e["margins"] += [("parameter_tolerance", d["step_norm"], ptol * (prob.x_norm(x) + ptol)),
                         ("function_tolerance", abs(e["cost_change"]), X.num(P["function_tolerance"]) * cost),
                         ("min_relative_decrease", e["rho"], P["min_relative_decrease"])]
        if d["step_norm"] <= ptol * (prob.x_norm(x) + ptol):
            term = TERM_PARAMETER
            log.append(e)
            break
        if abs(e["cost_change"]) <= X.num(P["function_tolerance"]) * cost:
            term = TERM_FUNCTION
            log.append(e)
            break
        if e["rho"] > P["min_relative_decrease"]:
            x = cand
            sys = prob.system(x)
            st = Strategy(prob, sys, scale)
            cost = sys["cost"]
            e["margins"] += [("decrease_threshold", e["rho"], P["decrease_threshold"]), ("increase_threshold", e["rho"], P["increase_threshold"]),
                             ("gradient_tolerance", st.grad_max, P["gradient_tolerance"])]
            if e["rho"] < P["decrease_threshold"]:
                radius = radius * X.num(0.5)
            if e["rho"] > P["increase_threshold"]:
                radius = max(radius, X.num(3.0) * d["dogleg_norm"])
            radius = min(X.num(P["max_radius"]), radius)
            mu = max(X.num(P["min_mu"]), X.num(2.0) * mu / X.num(P["mu_increase_factor"]))
            reuse = False
            e.update(accepted=1, cost=cost, gradient_max_norm=st.grad_max)
            log.append(e)
            if st.grad_max <= P["gradient_tolerance"]:
                term = TERM_GRADIENT
        else:
            radius, reuse = radius * X.num(0.5), True
            log.append(e)
            if radius < P["min_radius"]:
                term = TERM_RADIUS
    out.update(x=x, log=log, termination=term, iterations=it, cost=cost, radius=radius, mu=mu)
    return out


def decisions(res):
    """the sequence a device run must reproduce: per entry (step kind, accepted, mu retries), then the termination"""
    return [(e["step_kind"], e["accepted"], e["mu_retries"]) for e in res["log"]], res["termination"], res["iterations"]


def min_margin(res_f, res_m):
    """over every decision of the float64 run: |value - threshold| / max(|value_f64 - value_mp|, tiny) -> (worst ratio, its name);
    the two runs must have the same shape"""
    worst, name = math.inf, None
    for ef, em in zip(res_f["log"], res_m["log"]):
        for (n, vf, tf), (_, vm, tm) in zip(ef["margins"], em["margins"]):
            dist = abs(float(vf) - float(vm)) + abs(float(tf) - float(tm))
            margin = abs(float(vm) - float(tm))
            ratio = margin / max(dist, 1e-300)
            if ratio < worst:
                worst, name = ratio, f"{n} at iteration {ef['iteration']}"
    return worst, name
