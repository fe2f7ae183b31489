"""Reference of the visual-inertial alignment (include/lvi_align.h): a restatement of tmp_pre_integration and
all_image_frame (estimator.cpp:99, :132-135, :1019-1033), the excitation check (:273-300), solveGyroscopeBias, TangentBasis,
RefineGravity, LinearAlignment and VisualIMUAlignment (initial/initial_aligment.cpp:3-209) and the tail of visualInitialAlign
with Utility::g2R (estimator.cpp:450-486).

The float64 statement is the one the library is held to BIT FOR BIT, so the order of every operation is spelt out on Python
floats: a chain of scalars and matrices is evaluated left to right (R_i' * dt * dt / 2 is ((R_i' dt) dt) / 2, a 3 x 3 product
element is a b + c d + e f from the left); the identity factors of the reference are exact and left out; r_A = tmp_A' tmp_A
is a dense sum, started at 0, over the six rows in ascending order; every entry of A and b takes its pairs in ascending pair
order, onto 0 or (refinement passes 1..3) onto the previous pass's scaled system, then is multiplied by 1000.0.  The symmetric
solve is the restatement's own, an unpivoted L D L' in natural order, stated twice: dense (`ldl_dense`) and on the band and
the border only (`ldl_band`); they give the same bits.  A second route solves the dense system with numpy.linalg.solve, and
the accuracy of all of them is measured in mpmath at 50 digits.  Nothing here reads the library."""
import math

import mpmath
import numpy as np

import preint_ref as PR
from marg_ref import F64

mpmath.mp.dps = 50
BAND, BW = 5, 6
NB_LINEAR, NB_REFINE, PASSES, SYSTEMS = 4, 3, 4, 5
OK, GRAVITY_NORM, NEGATIVE_SCALE, NEGATIVE_SCALE_REFINED, SINGULAR, TOO_FEW = range(6)
REASONS = ("OK", "GRAVITY_NORM", "NEGATIVE_SCALE", "NEGATIVE_SCALE_REFINED", "SINGULAR", "TOO_FEW")
APPLY_OPPOSITE = 1
PARAMS = dict(PR.PARAMS, TIC=(0.0, 0.0, 0.0))
MAX_FRAMES = 256
DBL_MAX = float(np.finfo(np.float64).max)
U = 2.0 ** -52


class CapacityError(Exception):
    pass


class StateError(Exception):
    pass


def positive_finite(v):
    return v > 0.0 and v <= DBL_MAX


def mat3_tmul(A, B):
    return [A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j] for i in range(3) for j in range(3)]


def mat3_tvec(A, v):
    return [A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2] for i in range(3)]


def rot_to_quat(R):
    """Eigen's Quaternion(Matrix3) -> x y z w"""
    q = [0.0] * 4
    t = R[0] + R[4] + R[8]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t
    else:
        i = 0
        if R[4] > R[0]:
            i = 1
        if R[8] > R[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[3 * k + j] - R[3 * j + k]) * t
        q[j] = (R[3 * j + i] + R[3 * i + j]) * t
        q[k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q


def quat_inv(q):
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return [-q[0] / n2, -q[1] / n2, -q[2] / n2, q[3] / n2]


def norm3(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def normalized3(v):
    n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    if n2 > 0.0:
        n = math.sqrt(n2)
        return [v[0] / n, v[1] / n, v[2] / n]
    return list(v)


# ---- solveGyroscopeBias ---------------------------------------------------------------------------------------------
def gyro_pair(Ri, Rj, delta_q, J):
    e = PR.quat_mul(quat_inv(delta_q), rot_to_quat(mat3_tmul(Ri, Rj)))
    tb = [2.0 * e[k] for k in range(3)]
    A = [[J[3 + r][12 + c] for c in range(3)] for r in range(3)]
    out = []
    for r in range(3):
        for c in range(3):
            out.append(A[0][r] * A[0][c] + A[1][r] * A[1][c] + A[2][r] * A[2][c])
    for r in range(3):
        out.append(A[0][r] * tb[0] + A[1][r] * tb[1] + A[2][r] * tb[2])
    return out


def ldl_dense(A, b):
    """unpivoted L D L' of the dense symmetric A (list of rows) -> (x or None, smallest pivot, L with d on its diagonal)"""
    n = len(b)
    A = [list(r) for r in A]
    mp = DBL_MAX
    for j in range(n):
        v = A[j][j]
        for k in range(j):
            l = A[j][k]
            v = v - (l * A[k][k]) * l
        if not positive_finite(v):
            return None, 0.0, A
        mp = min(mp, v)
        for i in range(j + 1, n):
            s = A[i][j]
            for k in range(j):
                s = s - (A[i][k] * A[k][k]) * A[j][k]
            A[i][j] = s / v
        A[j][j] = v
    x = list(b)
    for i in range(n):
        z = x[i]
        for k in range(i):
            z = z - A[i][k] * x[k]
        x[i] = z
    for i in range(n):
        x[i] = x[i] / A[i][i]
    for i in range(n - 1, -1, -1):
        z = x[i]
        for k in range(i + 1, n):
            z = z - A[k][i] * x[k]
        x[i] = z
    return x, mp, A


def in_pattern(nd, i, k):
    """L[i][k], k < i, lies inside the band or the border"""
    return i >= nd or i - k <= BAND


def ldl_band(A, b, nd):
    """the same factorisation over the entries inside the pattern only: what the library computes"""
    n = len(b)
    if 2 * (nd - 3) < n:                                     # 6 (F - 1) equations for n unknowns
        return None, 0.0
    A = [list(r) for r in A]
    lo = lambda j: (max(0, j - BAND) if j < nd else 0)
    mp = DBL_MAX
    for j in range(n):
        v = A[j][j]
        for k in range(lo(j), j):
            l = A[j][k]
            v = v - (l * A[k][k]) * l
        if not positive_finite(v):
            return None, 0.0
        mp = min(mp, v)
        for i in range(j + 1, n):
            if not in_pattern(nd, i, j):
                continue
            s = A[i][j]
            for k in range(max(lo(i), lo(j)), j):
                s = s - (A[i][k] * A[k][k]) * A[j][k]
            A[i][j] = s / v
        A[j][j] = v
    x = list(b)
    for i in range(n):
        z = x[i]
        for k in range(lo(i), i):
            z = z - A[i][k] * x[k]
        x[i] = z
    for i in range(n):
        x[i] = x[i] / A[i][i]
    for i in range(n - 1, -1, -1):
        z = x[i]
        for k in range(i + 1, n):
            if in_pattern(nd, k, i):
                z = z - A[k][i] * x[k]
        x[i] = z
    return x, mp


# ---- TangentBasis, the pairs of LinearAlignment and RefineGravity ---------------------------------------------------
def tangent_basis(g0):
    """-> lxly as three rows of two"""
    a = normalized3(g0)
    t = [0.0, 0.0, 1.0]
    if a == t:
        t = [1.0, 0.0, 0.0]
    d = a[0] * t[0] + a[1] * t[1] + a[2] * t[2]
    b = normalized3([t[k] - a[k] * d for k in range(3)])
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    return [[b[k], c[k]] for k in range(3)]


def pair_system(fi, fj, TIC, lxly=None, g0=None):
    """one pair -> (r_A as rows, r_b); 10 wide without lxly, 9 with"""
    nb = NB_REFINE if lxly is not None else NB_LINEAR
    Wd = 6 + nb
    Ri, Rj, Ti, Tj = fi["R"], fj["R"], fi["T"], fj["T"]
    dt = fj["sum_dt"]
    tA = [[0.0] * Wd for _ in range(6)]
    tb = [0.0] * 6
    Rij = mat3_tmul(Ri, Rj)
    M = [Ri[3 * c + r] * dt * dt / 2 for r in range(3) for c in range(3)]
    Md = [Ri[3 * c + r] * dt for r in range(3) for c in range(3)]
    u = mat3_tvec(Ri, [Tj[k] - Ti[k] for k in range(3)])
    v = PR.mat3_vec(Rij, TIC)
    for r in range(3):
        tA[r][r] = -dt
        tA[3 + r][r] = -1.0
        for c in range(3):
            tA[3 + r][3 + c] = Rij[3 * r + c]
        tA[r][Wd - 1] = u[r] / 100.0
        tb[r] = fj["delta_p"][r] + v[r] - TIC[r]
        tb[3 + r] = fj["delta_v"][r]
        if lxly is None:
            for c in range(3):
                tA[r][6 + c] = M[3 * r + c]
                tA[3 + r][6 + c] = Md[3 * r + c]
        else:
            for c in range(2):
                tA[r][6 + c] = M[3 * r] * lxly[0][c] + M[3 * r + 1] * lxly[1][c] + M[3 * r + 2] * lxly[2][c]
                tA[3 + r][6 + c] = Md[3 * r] * lxly[0][c] + Md[3 * r + 1] * lxly[1][c] + Md[3 * r + 2] * lxly[2][c]
            tb[r] = tb[r] - (M[3 * r] * g0[0] + M[3 * r + 1] * g0[1] + M[3 * r + 2] * g0[2])
            tb[3 + r] = tb[3 + r] - (Md[3 * r] * g0[0] + Md[3 * r + 1] * g0[1] + Md[3 * r + 2] * g0[2])
    rA = [[0.0] * Wd for _ in range(Wd)]
    rb = [0.0] * Wd
    for a in range(Wd):
        for c in range(Wd):
            s = 0.0
            for k in range(6):
                s = s + tA[k][a] * tA[k][c]
            rA[a][c] = s
        s = 0.0
        for k in range(6):
            s = s + tA[k][a] * tb[k]
        rb[a] = s
    return rA, rb


def scatter(A, b, p, nd, nb, rA, rb):
    """pair p onto the dense A and b, as :167-174 / :105-112 place the blocks"""
    idx = list(range(3 * p, 3 * p + 6)) + list(range(nd, nd + nb))
    for a in range(6 + nb):
        for c in range(6 + nb):
            A[idx[a]][idx[c]] = A[idx[a]][idx[c]] + rA[a][c]
        b[idx[a]] = b[idx[a]] + rb[a]


def linear_gate(x, G):
    n = len(x)
    g = [x[n - 4 + k] for k in range(3)]
    s = x[n - 1] / 100.0
    gn = norm3(G)
    a = normalized3(g)
    g0 = [a[k] * gn for k in range(3)]
    reason = GRAVITY_NORM if abs(norm3(g) - gn) > 1.0 else NEGATIVE_SCALE if s < 0 else OK
    return reason, g, s, g0


def refine_step(x, lxly, G, g0):
    n = len(x)
    dg0, dg1, gn = x[n - 3], x[n - 2], norm3(G)
    a = normalized3([g0[k] + (lxly[k][0] * dg0 + lxly[k][1] * dg1) for k in range(3)])
    return [a[k] * gn for k in range(3)]


def linear_alignment(frames, TIC, G, solver="band"):
    """frames: dicts of R [9], T [3], sum_dt, delta_p, delta_v (frame 0 needs R and T only).  solver: "band", "dense" (the two
    statements of the L D L') or "numpy" (numpy.linalg.solve on the dense system, no pivot test).
    -> dict(reason, s, g_linear, g, x, n_state, systems [(A, b, x)], min_pivot [5])"""
    F = len(frames)
    nd = 3 * F
    TIC, G = [float(t) for t in TIC], [float(t) for t in G]
    out = dict(reason=OK, s=0.0, g_linear=[0.0] * 3, g=[0.0] * 3, x=[0.0] * (nd + NB_LINEAR), n_state=nd + NB_LINEAR, systems=[], min_pivot=[0.0] * SYSTEMS)
    g0, lxly, A, b = [0.0] * 3, None, None, None

    def solve(A, b):
        if solver == "band":
            return ldl_band(A, b, nd)
        if solver == "dense":
            return ldl_dense(A, b)[:2] if 2 * (nd - 3) >= len(b) else (None, 0.0)
        if 2 * (nd - 3) < len(b) or not np.all(np.isfinite(A)):
            return None, 0.0
        return [float(t) for t in np.linalg.solve(np.array(A), np.array(b))], float("nan")

    for w in range(SYSTEMS):
        nb = NB_LINEAR if w == 0 else NB_REFINE
        n = nd + nb
        if w < 2:
            A, b = [[0.0] * n for _ in range(n)], [0.0] * n
        if w >= 1:
            lxly = tangent_basis(g0)
        for p in range(F - 1):
            rA, rb = pair_system(frames[p], frames[p + 1], TIC, lxly if w >= 1 else None, g0)
            scatter(A, b, p, nd, nb, rA, rb)
        A = [[t * 1000.0 for t in row] for row in A]
        b = [t * 1000.0 for t in b]
        x, out["min_pivot"][w] = solve(A, b)
        if x is not None and not all(abs(t) <= DBL_MAX for t in x):      # a right-hand side that is not finite
            x = None
        out["systems"].append(([list(r) for r in A], list(b), list(x) if x is not None else [0.0] * n))      # copies: the next pass adds onto A and b
        if x is None:
            out["min_pivot"][w] = 0.0
            out.update(reason=SINGULAR, s=0.0, g_linear=[0.0] * 3, g=[0.0] * 3, x=[0.0] * (nd + NB_LINEAR), n_state=nd + NB_LINEAR)
            return out
        if w == 0:
            reason, g, s, g0 = linear_gate(x, G)
            out.update(reason=reason, g_linear=g, g=g, s=s, x=list(x), n_state=n)
            if reason != OK:
                return out
        else:
            g0 = refine_step(x, lxly, G, g0)
    x[n - 1] = x[n - 1] / 100.0
    out["systems"][-1] = (out["systems"][-1][0], out["systems"][-1][1], list(x))
    out.update(x=list(x), n_state=n, s=x[n - 1], g=g0)
    if out["s"] < 0.0:
        out["reason"] = NEGATIVE_SCALE_REFINED
    return out


def excitation(frames):
    """estimator.cpp:273-300 with sum_g started at 0; frames: those after the first"""
    m = len(frames)
    sm = [0.0] * 3
    for f in frames:
        for k in range(3):
            sm[k] = sm[k] + f["delta_v"][k] / f["sum_dt"]
    aver = [sm[k] * 1.0 / m for k in range(3)]
    var = 0.0
    for f in frames:
        d = [f["delta_v"][k] / f["sum_dt"] - aver[k] for k in range(3)]
        var = var + (d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return math.sqrt(var / m)


# ---- the handle: all_image_frame and tmp_pre_integration ------------------------------------------------------------
class Aligner:
    """the state and the operations of include/lvi_align.h in float64"""

    def __init__(self, max_frames=MAX_FRAMES, max_samples=PR.MAX_SAMPLES, **params):
        self.max_frames, self.max_samples = max_frames, max_samples
        self.P = dict(PARAMS)
        self.P.update(params)
        self.clear()

    def clear(self):
        self.frames, self.pending, self.have_imu = [], None, False
        self.acc_0, self.gyr_0 = [0.0] * 3, [0.0] * 3
        self.last = None

    def _fresh(self, Ba, Bg):
        return dict(state=PR.new_state(self.acc_0, self.gyr_0, Ba, Bg, F64), samples=[])

    def push_imu(self, dt, acc, gyr):
        n = len(dt)
        if self.pending is not None and len(self.pending["samples"]) + n > self.max_samples:
            raise CapacityError()
        q = PR.noise_diag(self.P, F64)
        for k in range(n):
            a, g = [float(t) for t in acc[k]], [float(t) for t in gyr[k]]
            if not self.have_imu:
                self.have_imu, self.acc_0, self.gyr_0 = True, a, g
            if self.pending is not None:
                PR.step(self.pending["state"], dt[k], acc[k], gyr[k], q, F64)
                self.pending["samples"].append((float(dt[k]), tuple(a), tuple(g)))
            self.acc_0, self.gyr_0 = a, g

    def add_frame(self, stamp, Ba, Bg):
        if len(self.frames) >= self.max_frames:
            raise CapacityError()
        if self.frames and not stamp > self.frames[-1]["stamp"]:
            raise ValueError("stamp")
        self.frames.append(dict(stamp=float(stamp), R=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], T=[0.0] * 3, key=False, pre=self.pending))
        self.pending = self._fresh(Ba, Bg)

    def erase_through(self, t0):
        at = [i for i, f in enumerate(self.frames) if f["stamp"] == t0]
        if not at:
            raise StateError()
        self.frames = self.frames[at[0] + 1:]

    def set_pose(self, stamp, R, T, key):
        at = [f for f in self.frames if f["stamp"] == stamp]
        if not at:
            raise StateError()
        at[0].update(R=[float(t) for t in np.asarray(R, np.float64).ravel()], T=[float(t) for t in T], key=bool(key))

    def record(self, i):
        """-> the frame's fields; the preintegration's are None for a frame without one"""
        f = self.frames[i]
        out = dict(stamp=f["stamp"], R=np.array(f["R"]), T=np.array(f["T"]), key=f["key"], samples=0, pre=None)
        if f["pre"] is not None:
            s = f["pre"]["state"]
            g = lambda v: np.array(v, dtype=np.float64)
            out.update(samples=len(f["pre"]["samples"]), pre=dict(sum_dt=float(s["sum_dt"]), delta_p=g(s["delta_p"]), delta_q=g(s["delta_q"]), delta_v=g(s["delta_v"]),
                       linearized_ba=g(s["linearized_ba"]), linearized_bg=g(s["linearized_bg"]), linearized_acc=g(s["linearized_acc"]),
                       linearized_gyr=g(s["linearized_gyr"]), jacobian=g(s["jacobian"])))
        return out

    def _lin(self, i):
        f = self.frames[i]
        d = dict(R=f["R"], T=f["T"])
        if i > 0:
            s = f["pre"]["state"]
            d.update(sum_dt=s["sum_dt"], delta_p=s["delta_p"], delta_v=s["delta_v"], delta_q=s["delta_q"], jacobian=s["jacobian"])
        return d

    def excitation(self):
        if len(self.frames) < 2:
            raise StateError()
        return excitation([self._lin(i) for i in range(1, len(self.frames))])

    def solve(self, Bgs, solver="band"):
        """VisualIMUAlignment -> (Bgs advanced [11, 3], info); info as linear_alignment's plus delta_bg and min_pivot [6]"""
        Bgs = np.array(Bgs, np.float64).reshape(11, 3)
        F = len(self.frames)
        info = dict(ok=False, reason=TOO_FEW, s=0.0, g_linear=[0.0] * 3, g=[0.0] * 3, x=[0.0] * (3 * F + 4), n_state=3 * F + 4, delta_bg=[0.0] * 3, systems=[],
                    min_pivot=[0.0] * 6, frames=F)
        if F < 2:
            return Bgs, info
        A, b = [0.0] * 9, [0.0] * 3
        fr = [self._lin(i) for i in range(F)]
        for p in range(F - 1):
            o = gyro_pair(fr[p]["R"], fr[p + 1]["R"], fr[p + 1]["delta_q"], fr[p + 1]["jacobian"])
            A = [A[k] + o[k] for k in range(9)]
            b = [b[k] + o[9 + k] for k in range(3)]
        dbg, mp, _ = ldl_dense([A[0:3], A[3:6], A[6:9]], b)
        info["gyro_system"] = (A, b)
        gyro_ok = dbg is not None and all(abs(t) <= DBL_MAX for t in dbg)
        info["min_pivot"][0] = mp
        if gyro_ok:
            info["delta_bg"] = dbg
        Bgs = np.array([[float(Bgs[i][k]) + info["delta_bg"][k] for k in range(3)] for i in range(11)])
        q = PR.noise_diag(self.P, F64)
        for f in self.frames[1:]:
            old = f["pre"]["state"]
            s = PR.new_state(old["linearized_acc"], old["linearized_gyr"], [0.0] * 3, [float(t) for t in Bgs[0]], F64)
            for dt, a, g in f["pre"]["samples"]:
                PR.step(s, dt, a, g, q, F64)
            f["pre"]["state"] = s
        if not gyro_ok:
            info["reason"] = SINGULAR
            return Bgs, info
        la = linear_alignment([self._lin(i) for i in range(F)], self.P["TIC"], self.P["G"], solver)
        info.update({k: la[k] for k in ("reason", "s", "g_linear", "g", "x", "n_state", "systems")})
        info["min_pivot"] = [mp] + la["min_pivot"]
        info["ok"] = la["reason"] == OK
        self.last = info
        return Bgs, info


# ---- the tail of visualInitialAlign ---------------------------------------------------------------------------------
class _MPX:
    sqrt, atan2, sin, cos, pi = staticmethod(mpmath.sqrt), staticmethod(mpmath.atan2), staticmethod(mpmath.sin), staticmethod(mpmath.cos), mpmath.pi
    num = staticmethod(lambda v: mpmath.mpf(float(v)))


class _FX:
    sqrt, atan2, sin, cos, pi = staticmethod(math.sqrt), staticmethod(math.atan2), staticmethod(math.sin), staticmethod(math.cos), math.pi
    num = staticmethod(float)


class _NPX:
    """the float64-numpy route of apply: the same formulas over numpy's matrix products"""
    sqrt, atan2, sin, cos, pi = staticmethod(np.sqrt), staticmethod(np.arctan2), staticmethod(np.sin), staticmethod(np.cos), np.pi
    num = staticmethod(np.float64)


def _yaw_left(deg, R, X):
    y = deg / X.num(180.0) * X.pi
    c, s = X.cos(y), X.sin(y)
    z, one = X.num(0.0), X.num(1.0)
    return PR.mat3_mul([c, -s, z, s, c, z, z, z, one], R)


def _yaw_deg(R, X):
    return X.atan2(R[3], R[0]) / X.pi * X.num(180.0)


def g2R(g, X):
    n = X.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
    a = [g[0] / n, g[1] / n, g[2] / n]
    c = a[2]
    flags = 0
    if c < X.num(-1.0 + 1e-12):
        q, flags = [X.num(1.0), X.num(0.0), X.num(0.0), X.num(0.0)], APPLY_OPPOSITE
    else:
        s = X.sqrt((X.num(1.0) + c) * X.num(2.0))
        inv = X.num(1.0) / s
        q = [a[1] * inv, -a[0] * inv, X.num(0.0) * inv, s * X.num(0.5)]
    Rq = PR.quat_to_rot(q, X)
    return _yaw_left(-_yaw_deg(Rq, X), Rq, X), flags


def apply(frame_count, TIC, Ps, Rs, x, g, key_R, X=_FX):
    """estimator.cpp:450-486 -> (Ps, Rs, Vs, g, rot_diff, flags) as nested lists of X's scalars"""
    N = X.num
    TIC, g, x = [N(t) for t in TIC], [N(t) for t in g], [N(t) for t in x]
    Ps = [[N(t) for t in np.asarray(p).ravel()] for p in Ps]
    Rs = [[N(t) for t in np.asarray(r).ravel()] for r in Rs]
    key_R = [[N(t) for t in np.asarray(r).ravel()] for r in key_R]
    s = x[-1]
    r0 = PR.mat3_vec(Rs[0], TIC)
    p0 = [s * Ps[0][k] - r0[k] for k in range(3)]
    for i in range(frame_count, -1, -1):
        ri = PR.mat3_vec(Rs[i], TIC)
        Ps[i] = [s * Ps[i][k] - ri[k] - p0[k] for k in range(3)]
    Vs = [[N(0.0)] * 3 for _ in range(frame_count + 1)]
    for kv in range(min(len(key_R), frame_count + 1)):
        Vs[kv] = PR.mat3_vec(key_R[kv], x[3 * kv:3 * kv + 3])
    R0, flags = g2R(g, X)
    rot = _yaw_left(-_yaw_deg(PR.mat3_mul(R0, Rs[0]), X), R0, X)
    g = PR.mat3_vec(rot, g)
    for i in range(frame_count + 1):
        Ps[i], Rs[i], Vs[i] = PR.mat3_vec(rot, Ps[i]), PR.mat3_mul(rot, Rs[i]), PR.mat3_vec(rot, Vs[i])
    return Ps, Rs, Vs, g, rot, flags


def apply_flat(res):
    """every number an apply returns, as one list"""
    Ps, Rs, Vs, g, rot, _ = res
    return [t for grp in (Ps, Rs, Vs) for row in grp for t in row] + list(g) + list(rot)


# ---- accuracy in mpmath -----------------------------------------------------------------------------------------------
def backward_error(A, b, x):
    """the normwise backward error |A x - b|_inf / (|A|_inf |x|_inf + |b|_inf) of float64 A, b, x, evaluated in mpmath"""
    n = len(b)
    M = mpmath.mpf
    r = max(abs(mpmath.fsum(M(A[i][k]) * M(x[k]) for k in range(n) if A[i][k] != 0.0) - M(b[i])) for i in range(n))
    an = max(mpmath.fsum(abs(M(t)) for t in row if t != 0.0) for row in A)
    return float(r / (an * max(abs(M(t)) for t in x) + max(abs(M(t)) for t in b)))


def solve_mp(A, b):
    """the solution in mpmath at 50 digits -> floats (rounded once)"""
    return [float(t) for t in mpmath.lu_solve(mpmath.matrix(A), mpmath.matrix(b))]


# ---- seeded scenes ----------------------------------------------------------------------------------------------------
def _rz(a):
    return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])


def _ry(a):
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1.0, 0], [-math.sin(a), 0, math.cos(a)]])


def _rx(a):
    return np.array([[1.0, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])


class Motion:
    """a smooth seeded trajectory: position and ZYX Euler angles are sums of two sines per axis; everything analytic"""

    def __init__(self, seed):
        rs = np.random.RandomState(seed)
        self.pa, self.pw, self.pp = rs.uniform(0.3, 1.0, (2, 3)), rs.uniform(0.8, 2.5, (2, 3)), rs.uniform(0, 6.28, (2, 3))
        self.ea, self.ew, self.ep = rs.uniform(0.1, 0.35, (2, 3)), rs.uniform(0.5, 1.6, (2, 3)), rs.uniform(0, 6.28, (2, 3))
        self.s = float(rs.uniform(0.5, 3.0))
        self.R_c0_w = _rz(rs.uniform(-3, 3)) @ _ry(rs.uniform(-0.6, 0.6)) @ _rx(rs.uniform(-0.6, 0.6))
        self.bg = rs.normal(0, 0.01, 3)
        self.tic = rs.normal(0, 0.05, 3)
        self.gw = np.array([0.0, 0.0, 9.8])

    def pos(self, t, d=0):
        ph = self.pw * t + self.pp
        f = {0: np.sin(ph), 1: self.pw * np.cos(ph), 2: -self.pw ** 2 * np.sin(ph)}[d]
        return (self.pa * f).sum(0)

    def eul(self, t, d=0):
        ph = self.ew * t + self.ep
        f = {0: np.sin(ph), 1: self.ew * np.cos(ph)}[d]
        return (self.ea * f).sum(0)                          # yaw, pitch, roll

    def rot(self, t):
        y, p, r = self.eul(t)
        return _rz(y) @ _ry(p) @ _rx(r)

    def gyr(self, t):
        (y, p, r), (yd, pd, rd) = self.eul(t), self.eul(t, 1)
        return np.array([rd - yd * math.sin(p), pd * math.cos(r) + yd * math.cos(p) * math.sin(r), -pd * math.sin(r) + yd * math.cos(p) * math.cos(r)])

    def acc(self, t):
        return self.rot(t).T @ (self.pos(t, 2) + self.gw)

    def pose(self, t):
        """R = R_c0_b, T = camera position in c0 / s"""
        Rwb = self.rot(t)
        return self.R_c0_w @ Rwb, self.R_c0_w @ (self.pos(t) + Rwb @ self.tic) / self.s

    def exact_pre(self, ti, tj):
        dt = tj - ti
        Ri = self.rot(ti)
        return dict(sum_dt=dt, delta_p=list(Ri.T @ (self.pos(tj) - self.pos(ti) - self.pos(ti, 1) * dt + 0.5 * self.gw * dt * dt)),
                    delta_v=list(Ri.T @ (self.pos(tj, 1) - self.pos(ti, 1) + self.gw * dt)))


def exact_frames(seed, F, frame_dt=0.1):
    """the frames of linear_alignment with analytic preintegrations -> (frames, motion)"""
    m = Motion(seed)
    out = []
    for i in range(F):
        R, T = m.pose(i * frame_dt)
        d = dict(R=[float(t) for t in R.ravel()], T=[float(t) for t in T])
        if i:
            d.update({k: (v if k == "sum_dt" else [float(t) for t in v]) for k, v in m.exact_pre((i - 1) * frame_dt, i * frame_dt).items()})
        out.append(d)
    return out, m


def imu_scene(seed, F, samples=4, frame_dt=0.1, counts=None, bias=True):
    """-> dict(motion, stamps, poses [(R, T)], imu [(dt, acc, gyr) per frame; frame 0's is the one sample that sets acc_0])"""
    m = Motion(seed)
    counts = [samples] * F if counts is None else list(counts)
    bg = m.bg if bias else np.zeros(3)
    stamps, poses, imu = [], [], []
    for i in range(F):
        t1 = i * frame_dt
        n = 1 if i == 0 else counts[i]
        h = frame_dt / max(n, 1)
        ts = [t1] if i == 0 else [t1 - frame_dt + h * (k + 1) for k in range(n)]
        imu.append((np.full(len(ts), h), np.array([m.acc(t) for t in ts]).reshape(-1, 3), np.array([m.gyr(t) + bg for t in ts]).reshape(-1, 3)))
        stamps.append(100.0 + t1)
        poses.append(m.pose(t1))
    return dict(motion=m, stamps=stamps, poses=poses, imu=imu, F=F)


def feed(al, sc, key=None):
    """a scene into an Aligner (or anything with its methods): IMU, frame, pose, in the estimator's order"""
    for i in range(sc["F"]):
        dt, acc, gyr = sc["imu"][i]
        if len(dt):
            al.push_imu(dt, acc, gyr)
        al.add_frame(sc["stamps"][i], np.zeros(3), np.zeros(3))
    for i in range(sc["F"]):
        R, T = sc["poses"][i]
        al.set_pose(sc["stamps"][i], R, T, True if key is None else key[i])


def same_frame(a, b):
    """None when two frame records hold the same values, else the first field that differs"""
    for k in ("stamp", "R", "T", "key", "samples"):
        if not np.array_equal(np.asarray(a[k], np.float64), np.asarray(b[k], np.float64), equal_nan=True):
            return k
    if (a["pre"] is None) != (b["pre"] is None):
        return "pre"
    if a["pre"] is not None:
        for k in a["pre"]:
            x, y = np.asarray(a["pre"][k], np.float64).reshape(-1), np.asarray(b["pre"][k], np.float64).reshape(-1)
            if not np.array_equal(x, y):
                bad = np.flatnonzero(x != y)
                return f"{k}[{bad[0]}]: {x[bad[0]]!r} != {y[bad[0]]!r} ({len(bad)} of {len(x)} differ)"
    return None


# ---- branch scenes: the same operations on the reference and on the library ------------------------------------------
class ZMotion(Motion):
    """motion along z only with identity rotations, R_c0_w = I, TIC 0 and no bias: the x and y parts of every system are exactly
    zero, so LinearAlignment's g is (0, 0, gz) and TangentBasis takes its other branch"""

    def __init__(self, seed):
        super().__init__(seed)
        self.pa[:, :2] = 0.0
        self.ea[:] = 0.0
        self.R_c0_w, self.bg, self.tic = np.eye(3), np.zeros(3), np.zeros(3)


BRANCHES = ("F2", "F3", "F4", "gnorm", "mirror", "gz", "nan", "zero_samples", "second", "erase", "keys", "neg_refined")
BGS0 = np.tile(np.array([1e-3, -2e-3, 5e-4]), (11, 1)) + np.arange(11)[:, None] * 1e-5


def branch_scene(name):
    """-> (scene, params, key flags or None, Bgs)"""
    F = {"F2": 2, "F3": 3, "F4": 4}.get(name, 8)
    counts = [4] * F
    if name == "zero_samples":
        counts[3] = 0
    if name == "erase":
        F, counts = 10, [3] * 10
    sc = imu_scene(40 + BRANCHES.index(name), F, counts=counts)
    params, key, Bgs = dict(TIC=tuple(float(t) for t in sc["motion"].tic)), None, BGS0
    if name == "gz":
        m = ZMotion(46)
        sc = imu_scene(46, F, counts=counts)
        sc["motion"] = m
        sc["poses"] = [m.pose(i * 0.1) for i in range(F)]
        sc["imu"] = [(d, np.array([m.acc(t) for t in np.r_[0.0, np.cumsum(d)][1:] + (0.0 if i == 0 else (i - 1) * 0.1)]).reshape(-1, 3), np.zeros((len(d), 3)))
                     for i, (d, _, _) in enumerate(sc["imu"])]
        params, Bgs = dict(TIC=(0.0, 0.0, 0.0)), np.zeros((11, 3))
    if name == "gnorm":
        params["G"] = (0.0, 0.0, 11.5)                       # | |g| - |G| | > 1 for a true gravity of 9.8
    if name == "mirror":
        sc["poses"] = [(R, -T) for R, T in sc["poses"]]
    if name == "nan":
        R3 = sc["poses"][3][0].copy()
        R3[0, 0] = float("nan")
        sc["poses"][3] = (R3, sc["poses"][3][1])
    if name == "keys":
        key = [i % 3 != 1 for i in range(F)]
    if name == "neg_refined":
        # translations unrelated to the motion leave s near 0 with either sign; of 300 seeds this is the first whose linear s
        # is positive (0.031) and whose refined s is negative (-0.234)
        sc = imu_scene(1011, F, counts=[3] * F)
        rs = np.random.RandomState(11)
        sc["poses"] = [(Rm, rs.normal(0, 1e-3, 3)) for Rm, _ in sc["poses"]]
        params = dict(TIC=tuple(float(t) for t in sc["motion"].tic))
    return sc, params, key, Bgs


def run_branch(name, make):
    """make(**params) -> an Aligner or an ImuAligner; -> (the handle, [(Bgs, info) of every solve])"""
    sc, params, key, Bgs = branch_scene(name)
    al = make(**params)
    feed(al, sc, key)
    if name == "erase":
        al.erase_through(sc["stamps"][2])
    outs = [al.solve(Bgs)]
    if name == "second":
        outs.append(al.solve(outs[0][0]))
    return al, outs


def check_solve(name, sv, reason, n_state, built, delta_bg, Bgs, s, g_linear, g, min_pivot, x, frames, systems):
    """one solve's outputs against the reference's, bit for bit (shared with the GPU tier)"""
    info = sv["info"]
    eq = lambda a, b: np.array_equal(np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel())
    assert (reason, n_state) == (info["reason"], info["n_state"]), (name, REASONS[reason], REASONS[info["reason"]])
    assert built == len(info["systems"]), (name, "built")
    assert eq(delta_bg, info["delta_bg"]), (name, "delta_bg", delta_bg, info["delta_bg"])
    assert eq(Bgs, sv["Bgs"]), (name, "Bgs")
    assert eq([s], [info["s"]]) and eq(g_linear, info["g_linear"]) and eq(g, info["g"]), (name, "s, g")
    assert eq(min_pivot, info["min_pivot"]), (name, "min_pivot", min_pivot, info["min_pivot"])
    assert eq(x[:n_state], info["x"][:n_state]), (name, "x")
    for i, (got, want) in enumerate(zip(frames, sv["frames"])):
        assert same_frame(want, got) is None, (name, i, same_frame(want, got))
    for w, ((A, b, xs), (Ar, br, xr)) in enumerate(zip(systems, info["systems"])):
        assert eq(A, Ar), (name, w, "A")
        assert eq(b, br) and eq(xs, xr), (name, w, "b, x")
