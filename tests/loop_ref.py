"""TEST INFRASTRUCTURE — restatement of the loop-closure registration (include/lvi_loop.h).

The ICP is pcl::IterativeClosestPoint<PointXYZI, PointXYZI> of PCL 1.12.1 as performLoopClosure configures it
(mapOptimization.cpp:579-590: setMaxCorrespondenceDistance, setMaximumIterations(100), setTransformationEpsilon(1e-6),
setEuclideanFitnessEpsilon(1e-6), setRANSACIterations(0) = no rejector), written down from the behaviour of
registration/impl/icp.hpp, correspondence_estimation.hpp, transformation_estimation_svd.hpp,
default_convergence_criteria.hpp and Eigen's umeyama.  PCL's source is not in the tree: parity of the device code is
against THIS file, not against PCL.

    icp(src, tgt, ..., precision="f32")   as PCL computes: f32 clouds, f32 transforms, f32 Umeyama, NN by squared f32 distance
    icp(src, tgt, ..., precision="f64")   the same loop in float64 throughout (the yardstick of the GPU tier)

nn: a callable (queries [m,3], targets [n,3]) -> (idx [m], sqd [m]); nn_exhaustive (any precision, lowest index on ties),
nn_kdtree (the oracle's kd-tree, f32) and nn_reranked (the kd-tree's five candidates re-ranked in float64) are given.

incremental_cloud (the one documented uncertainty, lvi_loop_params): True = every iteration transforms the already
transformed cloud by that iteration's step (icp.hpp's transformCloud on input_transformed); False = the original cloud by
the composed final transformation.

Never imported by the product package."""
import ctypes as C

import numpy as np

F32, F64 = np.float32, np.float64
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
OK, TOO_FEW_POINTS, NO_CORR = 0, 1, 2
DBL_MAX = np.finfo(np.float64).max


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def sqd(a, b):
    """(dx*dx + dy*dy) + dz*dz in the arrays' own precision"""
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nn_exhaustive(q, t, chunk=256):
    idx = np.zeros(len(q), np.int64)
    best = np.zeros(len(q), q.dtype)
    for a in range(0, len(q), chunk):
        d = sqd(q[a:a + chunk, None, :], t[None, :, :])
        idx[a:a + chunk] = np.argmin(d, axis=1)                       # the first (lowest index) of equal distances
        best[a:a + chunk] = d[np.arange(d.shape[0]), idx[a:a + chunk]]
    return idx, best


def _kd5(oracle, q32, t32):
    idx = np.full((len(q32), 5), -1, np.int32)
    d = np.zeros((len(q32), 5), F32)
    oracle.dll.lvo_test_kdtree_knn(_p(t32), len(t32), _p(q32), len(q32), _p(idx), _p(d))
    return idx, d


def nn_kdtree(oracle):
    def f(q, t):
        q32, t32 = np.ascontiguousarray(q, F32), np.ascontiguousarray(t, F32)
        idx, d = _kd5(oracle, q32, t32)
        return idx[:, 0].astype(np.int64), d[:, 0].astype(q.dtype)
    return f


def nn_reranked(oracle):
    """float64 nearest neighbour among the five f32 candidates of the kd-tree (they differ from the exact float64 answer
    only where the sixth f32 neighbour is nearer in float64 than the five: never on clouds whose points are leaf-sized apart)"""
    def f(q, t):
        q32, t32 = np.ascontiguousarray(q, F32), np.ascontiguousarray(t, F32)
        idx, _ = _kd5(oracle, q32, t32)
        ok = idx >= 0
        cand = t[np.maximum(idx, 0)]                                   # [m, 5, 3] in t's precision
        d = np.where(ok, sqd(q[:, None, :], cand), np.inf)
        k = np.argmin(d, axis=1)
        r = np.arange(len(q))
        return idx[r, k].astype(np.int64), d[r, k]
    return f


def transform(T, p):
    """((m0 x + m1 y) + m2 z) + m3 per row, in T's / p's precision (lvi_loop.hip's apply16)"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def compose(A, B):
    """A @ B with the device's association ((a0 b0 + a1 b1) + a2 b2) + a3 b3, in the arrays' precision"""
    out = np.zeros((4, 4), A.dtype)
    for i in range(4):
        for j in range(4):
            out[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return out


def umeyama(P, Q):
    """Eigen::umeyama(src = P, dst = Q, with_scaling = false) in the arrays' precision: (T 4x4, reflected)"""
    dt = P.dtype
    n = len(P)
    mp, mq = P.mean(axis=0, dtype=dt), Q.mean(axis=0, dtype=dt)
    sigma = ((Q - mq).T @ (P - mp)) / dt.type(n)
    U, _, Vt = np.linalg.svd(sigma)
    reflected = bool(np.linalg.det(U.astype(F64)) * np.linalg.det(Vt.astype(F64)) < 0)
    S = np.ones(3, dt)
    if reflected:
        S[2] = -1
    R = ((U * S[None, :]) @ Vt).astype(dt)
    T = np.eye(4, dtype=dt)
    T[:3, :3] = R
    T[:3, 3] = mq - R @ mp
    return T, reflected


class Criteria:
    """pcl::registration::DefaultConvergenceCriteria with ICP's settings: max similar iterations 0, absolute MSE 1e-12"""

    def __init__(self, max_iters=100, transformation_epsilon=1e-6, fitness_epsilon=1e-6):
        self.max_iters, self.teps, self.feps = int(max_iters), float(transformation_epsilon), float(fitness_epsilon)
        self.iterations = 0
        self.prev_mse = DBL_MAX
        self.mse = 0.0
        self.state = NOT_CONVERGED

    def has_converged(self, step, kept_sqd):
        """step: this iteration's 4x4; kept_sqd: the kept correspondences' squared distances.  Called after ++iterations."""
        self.iterations += 1
        dt = step.dtype.type
        cos = 0.5 * float(((step[0, 0] + step[1, 1]) + step[2, 2]) - dt(1))
        tsq = float((step[0, 3] * step[0, 3] + step[1, 3] * step[1, 3]) + step[2, 3] * step[2, 3])
        self.mse = float(np.sum(np.asarray(kept_sqd, F64))) / len(kept_sqd)
        self.state = NOT_CONVERGED
        if self.iterations >= self.max_iters:
            self.state = ITERATIONS
        elif cos >= 1.0 - self.teps and tsq <= self.teps:
            self.state = TRANSFORM
        elif self.mse < 1e-12:
            self.state = ABS_MSE
        elif abs(self.mse - self.prev_mse) / self.prev_mse < self.feps:
            self.state = REL_MSE
        else:
            self.prev_mse = self.mse
        return self.state != NOT_CONVERGED


def icp(src, tgt, nn, max_corr_dist=30.0, max_iters=100, transformation_epsilon=1e-6, fitness_epsilon=1e-6, precision="f32",
        incremental_cloud=True, min_source=0, min_target=0, fitness_nn=None):
    """src, tgt: [n, 3].  -> dict(status, T, converged, state, iterations, fitness, n_corr, mse, aligned)"""
    dt = F32 if precision == "f32" else F64
    src, tgt = np.ascontiguousarray(src, dt), np.ascontiguousarray(tgt, dt)
    out = dict(status=OK, T=np.eye(4, dtype=dt), converged=False, state=NOT_CONVERGED, iterations=0, fitness=DBL_MAX, n_corr=0, mse=0.0, aligned=src.copy())
    if len(src) < max(min_source, 1) or len(tgt) < max(min_target, 1):
        out["status"] = TOO_FEW_POINTS
        return out
    max2 = float(F32(max_corr_dist)) ** 2
    crit = Criteria(max_iters, transformation_epsilon, fitness_epsilon)
    final = np.eye(4, dtype=dt)
    cur = src.copy()
    while True:
        idx, d = nn(cur, tgt)
        keep = d.astype(F64) <= max2
        out["n_corr"] = int(keep.sum())
        if out["n_corr"] < 3:
            out["status"] = NO_CORR
            crit.state = NO_CORRESPONDENCES
            break
        step, _ = umeyama(cur[keep], tgt[idx[keep]])
        final = compose(step, final)
        cur = transform(step, cur) if incremental_cloud else transform(final, src)
        if crit.has_converged(step, d[keep]):
            out["converged"] = True
            break
    idx, d = (fitness_nn or nn)(cur, tgt)
    out.update(T=final, state=crit.state, iterations=crit.iterations, mse=crit.mse, aligned=cur, fitness=float(np.sum(d.astype(F64))) / len(cur))
    return out


# ---- the host side of performLoopClosure (:592-627) in float64 numpy -------------------------------------------------
def rpy_matrix(x, y, z, roll, pitch, yaw):
    """pcl::getTransformation(x, y, z, roll, pitch, yaw) as a 4x4 float64"""
    A, B, Cc, D, E, F = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    T = np.eye(4)
    T[:3, :3] = [[A * Cc, A * D * F - B * E, B * F + A * D * E], [B * Cc, A * E + B * D * F, B * D * E - A * F], [-D, Cc * F, Cc * E]]
    T[:3, 3] = [x, y, z]
    return T


def euler_of(T):
    """pcl::getTranslationAndEulerAngles: (x, y, z, roll, pitch, yaw)"""
    return (T[0, 3], T[1, 3], T[2, 3], np.arctan2(T[2, 1], T[2, 2]), np.arcsin(-T[2, 0]), np.arctan2(T[1, 0], T[0, 0]))


def constraint(correction, pose_cur, pose_pre):
    """poseFrom.between(poseTo) of :603-614 as a 4x4 float64: poses are (roll, pitch, yaw, x, y, z) of the two keys,
    correction the ICP's final transformation.  tCorrect = correction * tWrong goes through its Euler angles, as the
    reference's gtsam::Pose3(Rot3::RzRyRx(roll, pitch, yaw), Point3(x, y, z)) does."""
    r, p, y, tx, ty, tz = [float(v) for v in pose_cur]
    t_wrong = rpy_matrix(tx, ty, tz, r, p, y)
    t_correct = np.asarray(correction, F64) @ t_wrong
    x, yy, z, roll, pitch, yaw = euler_of(t_correct)
    pose_from = rpy_matrix(x, yy, z, roll, pitch, yaw)
    r, p, y, tx, ty, tz = [float(v) for v in pose_pre]
    pose_to = rpy_matrix(tx, ty, tz, r, p, y)
    return np.linalg.inv(pose_from) @ pose_to


def rot_angle(Ra, Rb):
    """the rotation angle of Ra^T Rb (radians), from the skew part as well as the trace: exact for tiny angles, where
    acos of the trace alone resolves nothing below 1e-8"""
    M = np.asarray(Ra, F64)[:3, :3].T @ np.asarray(Rb, F64)[:3, :3]
    s = 0.5 * np.sqrt((M[2, 1] - M[1, 2]) ** 2 + (M[0, 2] - M[2, 0]) ** 2 + (M[1, 0] - M[0, 1]) ** 2)
    return float(np.arctan2(s, (np.trace(M) - 1.0) / 2.0))
