"""Reference of the IMU preintegration (include/lvi_preint.h): a restatement of IntegrationBase
(factor/integration_base.h:9-158: the constructor, push_back, propagate, midPointIntegration, repropagate), of
Estimator::processIMU (estimator.cpp:82-116) and of the preintegration side of Estimator::slideWindow (:988-1016,
:1043-1068), in two arithmetics from the same float64 inputs: Python float64 (`F64`) and mpmath at 50 digits (`MP`).

The float64 run is the statement the library is held to BIT FOR BIT, so the order of every operation is spelt out on
scalars: a chain of scalars and matrices is evaluated left to right (-0.25 * R0 * A0 * dt * dt is (((-0.25 R0) A0) dt) dt, a
3 x 3 product element is a b + c d + e f from the left), and every element of F jacobian, F covariance, T F' and
V noise V' is a sum, started at 0, over the structurally non-zero terms of F (or of V) in ascending k; a term of the last
product is (V[r][k] q[k]) V[c][k].  Nothing here reads the library."""
import numpy as np

import win_ref as W
from marg_ref import F64, MP  # noqa: F401

SLOTS, WINDOW, MAX_SAMPLES, CHUNK = 11, 10, 8192, 16
N, NV = 15, 18
PARAMS = dict(acc_n=0.08, gyr_n=0.004, acc_w=0.00004, gyr_w=2.0e-6, G=(0.0, 0.0, 9.8))


class CapacityError(Exception):
    pass


class StateError(Exception):
    pass


def _block_masks():
    f, v = [], []
    for r in range(N):
        b, i = divmod(r, 3)
        f.append({0: {i, 3, 4, 5, 6 + i} | set(range(9, 15)), 1: {3, 4, 5, 12 + i}, 2: {3, 4, 5, 6 + i} | set(range(9, 15)), 3: {9 + i}, 4: {12 + i}}[b])
        v.append({0: set(range(12)), 1: {3 + i, 9 + i}, 2: set(range(12)), 3: {12 + i}, 4: {15 + i}}[b])
    return [sorted(s) for s in f], [sorted(s) for s in v]


FMASK, VMASK = _block_masks()                    # the structurally non-zero columns of every row of F (:90-105) and V (:108-120)


def noise_diag(P, X):
    an, gn, aw, gw = (X.num(P[k]) for k in ("acc_n", "gyr_n", "acc_w", "gyr_w"))
    return [an * an] * 3 + [gn * gn] * 3 + [an * an] * 3 + [gn * gn] * 3 + [aw * aw] * 3 + [gw * gw] * 3


def quat_to_rot(q, X):
    """Eigen's toRotationMatrix of the quaternion as it stands, in the order of csrc/lvi_marg_math.hpp -> 9 scalars, row-major"""
    x, y, z, w = q
    two, one = X.num(2.0), X.num(1.0)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return [one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)]


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def mat3_vec(A, v):
    return [A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2] for i in range(3)]


def mat3_mul(A, B):
    return [A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)]


def skew(v, X):
    z = X.num(0.0)
    return [z, -v[2], v[1], v[2], z, -v[0], -v[1], v[0], z]


def new_state(acc_0, gyr_0, ba, bg, X):
    """the constructor (:13-18)"""
    z, one = X.num(0.0), X.num(1.0)
    A = lambda v: [X.num(t) for t in v]
    return dict(sum_dt=z, delta_p=[z, z, z], delta_q=[z, z, z, one], delta_v=[z, z, z], linearized_ba=A(ba), linearized_bg=A(bg), acc_0=A(acc_0), gyr_0=A(gyr_0),
                linearized_acc=A(acc_0), linearized_gyr=A(gyr_0), jacobian=[[one if r == c else z for c in range(N)] for r in range(N)],
                covariance=[[z] * N for _ in range(N)])


def step(s, dt, acc_1, gyr_1, q, X):
    """one propagate (:130-158) of the state s, in place"""
    half, quarter, two, one, zero = X.num(0.5), X.num(0.25), X.num(2.0), X.num(1.0), X.num(0.0)
    dt = X.num(dt)
    acc_1, gyr_1 = [X.num(t) for t in acc_1], [X.num(t) for t in gyr_1]
    ba, bg = s["linearized_ba"], s["linearized_bg"]
    a0 = [s["acc_0"][k] - ba[k] for k in range(3)]
    a1 = [acc_1[k] - ba[k] for k in range(3)]
    w = [half * (s["gyr_0"][k] + gyr_1[k]) - bg[k] for k in range(3)]
    R0 = quat_to_rot(s["delta_q"], X)
    un_acc_0 = mat3_vec(R0, a0)
    rq = quat_mul(s["delta_q"], [w[0] * dt / two, w[1] * dt / two, w[2] * dt / two, one])
    R1 = quat_to_rot(rq, X)                      # un-normalised, as Eigen's toRotationMatrix reads result_delta_q
    un_acc_1 = mat3_vec(R1, a1)
    dp, dv = list(s["delta_p"]), list(s["delta_v"])
    for k in range(3):
        un_acc = half * (un_acc_0[k] + un_acc_1[k])
        dp[k] = s["delta_p"][k] + s["delta_v"][k] * dt + half * un_acc * dt * dt
        dv[k] = s["delta_v"][k] + un_acc * dt
    n = X.sqrt(rq[0] * rq[0] + rq[1] * rq[1] + rq[2] * rq[2] + rq[3] * rq[3])
    # ---- F and V (:90-120): only the structurally non-zero entries are ever written or read
    A0, A1, Wm = skew(a0, X), skew(a1, X), skew(w, X)
    F = [[None] * N for _ in range(N)]
    V = [[None] * NV for _ in range(N)]
    mq, mh = -quarter, -half
    for i in range(3):
        r0, r1 = R0[3 * i:3 * i + 3], R1[3 * i:3 * i + 3]
        x1q = [(mq * r1[0]) * A1[k] + (mq * r1[1]) * A1[3 + k] + (mq * r1[2]) * A1[6 + k] for k in range(3)]
        x1h = [(mh * r1[0]) * A1[k] + (mh * r1[1]) * A1[3 + k] + (mh * r1[2]) * A1[6 + k] for k in range(3)]
        for j in range(3):
            K = [(one if k == j else zero) - Wm[3 * k + j] * dt for k in range(3)]
            x0q = (mq * r0[0]) * A0[j] + (mq * r0[1]) * A0[3 + j] + (mq * r0[2]) * A0[6 + j]
            x0h = (mh * r0[0]) * A0[j] + (mh * r0[1]) * A0[3 + j] + (mh * r0[2]) * A0[6 + j]
            x1qK = x1q[0] * K[0] + x1q[1] * K[1] + x1q[2] * K[2]
            x1hK = x1h[0] * K[0] + x1h[1] * K[1] + x1h[2] * K[2]
            F[i][3 + j] = x0q * dt * dt + x1qK * dt * dt
            F[i][9 + j] = (mq * (r0[j] + r1[j])) * dt * dt
            F[i][12 + j] = x1q[j] * dt * dt * -dt
            F[3 + i][3 + j] = K[i]
            F[6 + i][3 + j] = x0h * dt + x1hK * dt
            F[6 + i][9 + j] = (mh * (r0[j] + r1[j])) * dt
            F[6 + i][12 + j] = x1h[j] * dt * -dt
            y1q = (quarter * -r1[0]) * A1[j] + (quarter * -r1[1]) * A1[3 + j] + (quarter * -r1[2]) * A1[6 + j]
            y1h = (half * -r1[0]) * A1[j] + (half * -r1[1]) * A1[3 + j] + (half * -r1[2]) * A1[6 + j]
            V[i][j] = (quarter * r0[j]) * dt * dt
            V[i][3 + j] = y1q * dt * dt * half * dt
            V[i][6 + j] = (quarter * r1[j]) * dt * dt
            V[i][9 + j] = V[i][3 + j]
            V[6 + i][j] = (half * r0[j]) * dt
            V[6 + i][3 + j] = y1h * dt * half * dt
            V[6 + i][6 + j] = (half * r1[j]) * dt
            V[6 + i][9 + j] = V[6 + i][3 + j]
        F[i][i] = one
        F[i][6 + i] = dt
        F[3 + i][12 + i] = -one * dt
        F[6 + i][6 + i] = one
        F[9 + i][9 + i] = one
        F[12 + i][12 + i] = one
        V[3 + i][3 + i] = half * dt
        V[3 + i][9 + i] = half * dt
        V[9 + i][12 + i] = dt
        V[12 + i][15 + i] = dt
    # ---- :124-125
    J, C = s["jacobian"], s["covariance"]

    def fdot(r, M, c):
        t = zero
        for k in FMASK[r]:
            t = t + F[r][k] * M[k][c]
        return t

    Jn = [[fdot(r, J, c) for c in range(N)] for r in range(N)]
    T = [[fdot(r, C, c) for c in range(N)] for r in range(N)]
    Cn = [[None] * N for _ in range(N)]
    for r in range(N):
        for c in range(N):
            t = zero
            for k in FMASK[c]:
                t = t + T[r][k] * F[c][k]
            u = zero
            for k in VMASK[r]:
                if k in VMASK[c]:
                    u = u + (V[r][k] * q[k]) * V[c][k]
            Cn[r][c] = t + u
    s.update(jacobian=Jn, covariance=Cn, delta_p=dp, delta_v=dv, delta_q=[rq[k] / n for k in range(4)], sum_dt=s["sum_dt"] + dt, acc_0=acc_1, gyr_0=gyr_1)


def nav_step(nav, acc_0, gyr_0, dt, acc, gyr, G, X):
    """estimator.cpp:105-112, in place: nav = dict(P, R [9], V, Ba, Bg)"""
    half, two, one = X.num(0.5), X.num(2.0), X.num(1.0)
    dt = X.num(dt)
    acc, gyr = [X.num(t) for t in acc], [X.num(t) for t in gyr]
    un_acc_0 = mat3_vec(nav["R"], [acc_0[k] - nav["Ba"][k] for k in range(3)])
    un_acc_0 = [un_acc_0[k] - G[k] for k in range(3)]
    th = [(half * (gyr_0[k] + gyr[k]) - nav["Bg"][k]) * dt for k in range(3)]
    nav["R"] = mat3_mul(nav["R"], quat_to_rot([th[0] / two, th[1] / two, th[2] / two, one], X))
    un_acc_1 = mat3_vec(nav["R"], [acc[k] - nav["Ba"][k] for k in range(3)])
    P, V = list(nav["P"]), list(nav["V"])
    for k in range(3):
        un_acc = half * (un_acc_0[k] + (un_acc_1[k] - G[k]))
        P[k] = nav["P"][k] + (dt * nav["V"][k] + half * dt * dt * un_acc)
        V[k] = nav["V"][k] + dt * un_acc
    nav["P"], nav["V"] = P, V


def to_record(s):
    """-> the fields of lvi_win_imu as float64 (an mpmath state is rounded)"""
    f = lambda v: np.array(v, dtype=object).astype(np.float64)
    return dict(sum_dt=float(s["sum_dt"]), delta_p=f(s["delta_p"]), delta_q=f(s["delta_q"]), delta_v=f(s["delta_v"]), linearized_ba=f(s["linearized_ba"]),
                linearized_bg=f(s["linearized_bg"]), jacobian=f(s["jacobian"]), covariance=f(s["covariance"]))


def exact_record(s):
    """the same fields as arrays of the state's own scalars"""
    return {k: (np.array(s[k], dtype=object) if isinstance(s[k], list) else s[k]) for k in ("sum_dt", "delta_p", "delta_q", "delta_v", "linearized_ba",
                                                                                            "linearized_bg", "jacobian", "covariance")}


def preintegrate(dts, accs, gyrs, ba, bg, X=F64, params=None):
    """as win_ref.preintegrate: the first sample initialises acc_0 and gyr_0, the others are pushed -> the state"""
    q = noise_diag(params or PARAMS, X)
    s = new_state(accs[0], gyrs[0], ba, bg, X)
    for dt, a, g in zip(dts[1:], accs[1:], gyrs[1:]):
        step(s, dt, a, g, q, X)
    return s


class Estimator:
    """the slots, first_imu, the navigation state and the operations of include/lvi_preint.h"""

    def __init__(self, X=F64, max_samples=MAX_SAMPLES, **params):
        self.X, self.max_samples = X, max_samples
        self.P = dict(PARAMS)
        self.P.update(params)
        self.clear()

    def clear(self):
        X = self.X
        z, one = X.num(0.0), X.num(1.0)
        self.slots = [None] * SLOTS                 # dict(state, samples [(dt, acc, gyr)])
        self.first_imu, self.acc_0, self.gyr_0 = False, [z] * 3, [z] * 3
        self.nav = dict(P=[z] * 3, R=[one, z, z, z, one, z, z, z, one], V=[z] * 3, Ba=[z] * 3, Bg=[z] * 3)

    def set_nav(self, P, R, V, Ba, Bg):
        A = lambda v: [self.X.num(t) for t in np.asarray(v, np.float64).ravel()]
        self.nav = dict(P=A(P), R=A(R), V=A(V), Ba=A(Ba), Bg=A(Bg))

    def nav_f64(self):
        f = lambda v: np.array(v, dtype=object).astype(np.float64)
        return dict(P=f(self.nav["P"]), R=f(self.nav["R"]).reshape(3, 3), V=f(self.nav["V"]), Ba=f(self.nav["Ba"]), Bg=f(self.nav["Bg"]))

    def _fresh(self):
        return dict(state=new_state(self.acc_0, self.gyr_0, self.nav["Ba"], self.nav["Bg"], self.X), samples=[])

    def push(self, frame_count, dt, acc, gyr):
        """n calls of processIMU"""
        X = self.X
        n = len(dt)
        if not 0 <= frame_count < SLOTS:
            raise ValueError("frame_count")
        if n == 0:
            return
        cur = self.slots[frame_count]
        if frame_count != 0 and (len(cur["samples"]) if cur else 0) + n > self.max_samples:
            raise CapacityError()
        q, G = noise_diag(self.P, X), [X.num(t) for t in self.P["G"]]
        for k in range(n):
            a, g = [X.num(t) for t in acc[k]], [X.num(t) for t in gyr[k]]
            if not self.first_imu:
                self.first_imu, self.acc_0, self.gyr_0 = True, a, g
            if self.slots[frame_count] is None:
                self.slots[frame_count] = self._fresh()
            if frame_count != 0:
                sl = self.slots[frame_count]
                step(sl["state"], dt[k], acc[k], gyr[k], q, X)
                sl["samples"].append((float(dt[k]), tuple(float(t) for t in acc[k]), tuple(float(t) for t in gyr[k])))
                nav_step(self.nav, self.acc_0, self.gyr_0, dt[k], acc[k], gyr[k], G, X)
            self.acc_0, self.gyr_0 = a, g

    def repropagate(self, Bas, Bgs, slots=None):
        """IntegrationBase::repropagate (:38-52) of the named slots (all by default) with Bas[slot], Bgs[slot]"""
        slots = list(range(SLOTS)) if slots is None else list(slots)
        if any(self.slots[i] is None for i in slots):
            raise StateError()
        q = noise_diag(self.P, self.X)
        for i in slots:
            sl = self.slots[i]
            old = sl["state"]
            s = new_state(old["linearized_acc"], old["linearized_gyr"], Bas[i], Bgs[i], self.X)
            for dt, a, g in sl["samples"]:
                step(s, dt, a, g, q, self.X)
            sl["state"] = s

    def slide_old(self):
        if not self.first_imu:
            raise StateError()
        self.slots = self.slots[1:] + [self._fresh()]

    def slide_new(self):
        a, b = self.slots[SLOTS - 2], self.slots[SLOTS - 1]
        if a is None or b is None:
            raise StateError()
        if len(a["samples"]) + len(b["samples"]) > self.max_samples:
            raise CapacityError()
        q = noise_diag(self.P, self.X)
        for dt, acc, gyr in b["samples"]:
            step(a["state"], dt, acc, gyr, q, self.X)
            a["samples"].append((dt, acc, gyr))
        self.slots[SLOTS - 1] = self._fresh()

    def record(self, slot):
        if self.slots[slot] is None:
            raise StateError()
        return to_record(self.slots[slot]["state"])

    def samples(self, slot):
        s = self.slots[slot]["samples"]
        return (np.array([t[0] for t in s], np.float64), np.array([t[1] for t in s], np.float64).reshape(-1, 3),
                np.array([t[2] for t in s], np.float64).reshape(-1, 3))


# ---- seeded samples ------------------------------------------------------------------------------------------
def samples(seed, n, dt=0.02, vary=False, zero_dt_at=None):
    """-> (dt [n], acc [n, 3], gyr [n, 3]): a body that holds against gravity and turns slowly, with sensor noise"""
    rs = np.random.RandomState(seed)
    a0, w0 = np.array([0.3, -0.2, 9.7]) + rs.normal(0, 0.5, 3), rs.normal(0, 0.1, 3)
    acc = a0 + rs.normal(0, 0.05, (n, 3))
    gyr = w0 + rs.normal(0, 0.01, (n, 3))
    dts = np.full(n, dt) * (rs.uniform(0.5, 1.5, n) if vary else 1.0)
    if zero_dt_at is not None and zero_dt_at < n:
        dts[zero_dt_at] = 0.0
    return dts, acc, gyr


def scene_intervals(seed, frames):
    """the IMU samples tests/win_scenes.py::make_scene draws for `frames` frames, drawn the same way -> (ba, bg, [(dts, accs, gyrs)])"""
    import marg_ref as M
    import win_scenes as S
    rs = np.random.RandomState(seed)
    ba, bg = rs.normal(0, 0.02, 3), rs.normal(0, 0.002, 3)
    pose = np.r_[rs.normal(0, 0.02, 3), M.rand_quat(rs, 0.05)]
    sb = np.r_[3.0, rs.normal(0, 0.05, 2), ba, bg]
    out = []
    for _ in range(frames - 1):
        Rk = M.rot(pose[3:])
        a0, w0 = Rk.T @ S.G + rs.normal(0, 0.5, 3), rs.normal(0, 0.1, 3)
        accs = [a0 + rs.normal(0, 0.05, 3) + ba for _ in range(S.FRAME_SAMPLES)]
        gyrs = [w0 + rs.normal(0, 0.01, 3) + bg for _ in range(S.FRAME_SAMPLES)]
        p = W.preintegrate([S.SAMPLE_DT] * S.FRAME_SAMPLES, accs, gyrs, ba, bg)
        dt = p["sum_dt"]
        new = np.r_[pose[:3] + sb[:3] * dt - 0.5 * S.G * dt * dt + Rk @ p["delta_p"], M.quat_mul(pose[3:], p["delta_q"])]
        new[3:] /= np.linalg.norm(new[3:])
        sb = np.r_[sb[:3] - S.G * dt + Rk @ p["delta_v"], ba + rs.normal(0, 1e-4, 3), bg + rs.normal(0, 1e-5, 3)]
        pose = new
        out.append(([S.SAMPLE_DT] * S.FRAME_SAMPLES, accs, gyrs, p))
    return ba, bg, out


def same_record(a, b):
    """None when two records hold the same values (-0.0 == 0.0), else the first field that differs"""
    for k in ("sum_dt", "delta_p", "delta_q", "delta_v", "linearized_ba", "linearized_bg", "jacobian", "covariance"):
        x, y = np.asarray(a[k], np.float64).reshape(-1), np.asarray(b[k], np.float64).reshape(-1)
        if not np.array_equal(x, y):
            bad = np.flatnonzero(x != y)
            return f"{k}[{bad[0]}]: {x[bad[0]]!r} != {y[bad[0]]!r} ({len(bad)} of {len(x)} differ)"
    return None
