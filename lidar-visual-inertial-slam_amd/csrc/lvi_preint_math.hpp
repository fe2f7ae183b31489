// IMU preintegration of the sliding window (include/lvi_preint.h), usable from host and device and compilable
// without HIP: IntegrationBase::midPointIntegration and propagate (integration_base.h:54-158) and the navigation step of
// Estimator::processIMU (estimator.cpp:105-112).  All double.  Quaternions are x y z w; a vector is rotated by the rotation
// matrix of the quaternion taken as it stands (Eigen's toRotationMatrix), so result_delta_q, which is normalised only after
// the step (:153), gives R1 un-normalised.
//
// The order of every sum is part of the contract (tests/preint_ref.py states the same operations term by term and the
// library is held to it bit for bit):
//   - a chain of scalars and matrices is evaluated left to right, as Eigen does: -0.25 * R0 * A0 * dt * dt is
//     (((-0.25 R0) A0) dt) dt, and a 3 x 3 product element is a b + c d + e f from the left;
//   - jacobian = F jacobian; T = F covariance; covariance = T F' + V noise V', the noise being diagonal, so a term of the
//     last product is (V[r][k] q[k]) V[c][k];
//   - every element of these products is a sum, started at 0, over the structurally non-zero terms of F (or of V) in
//     ascending k: fmask(r) and vmask(r) name them.  Entries of F and V outside the masks are never written and never read.
#pragma once
#include "lvi_imu_math.hpp"

namespace lvi_preint_math {

using lvi_imu_math::quat_mul;
using lvi_marg_math::mat3_mul;
using lvi_marg_math::mat3_vec;
using lvi_marg_math::quat_to_rot;
using lvi_marg_math::skew;

constexpr int N = 15, NV = 18;                   // F is N x N, V is N x NV, both row-major

// the part of an IntegrationBase the vector chain carries; jacobian and covariance are kept beside it
struct State {
    double sum_dt, delta_p[3], delta_q[4], delta_v[3], linearized_ba[3], linearized_bg[3], acc_0[3], gyr_0[3];
};
// Ps / Rs / Vs / Bas / Bgs [j] of the slot being pushed; R row-major
struct Nav {
    double P[3], R[9], V[3], Ba[3], Bg[3];
};
// what one step leaves for F and V: 28 doubles
struct StepGeom {
    double dt, R0[9], R1[9], w[3], a0[3], a1[3];
};

// the structurally non-zero columns of row r of F (:90-105) and of V (:108-120)
LVI_MARG_HD constexpr unsigned fmask(int r)
{
    const int b = r / 3, i = r % 3;
    return b == 0 ? ((1u << i) | (7u << 3) | (1u << (6 + i)) | (63u << 9))
         : b == 1 ? ((7u << 3) | (1u << (12 + i)))
         : b == 2 ? ((7u << 3) | (1u << (6 + i)) | (63u << 9))
         : b == 3 ? (1u << (9 + i))
                  : (1u << (12 + i));
}
LVI_MARG_HD constexpr unsigned vmask(int r)
{
    const int b = r / 3, i = r % 3;
    return b == 0 || b == 2 ? 0xfffu : b == 1 ? ((1u << (3 + i)) | (1u << (9 + i))) : b == 3 ? (1u << (12 + i)) : (1u << (15 + i));
}

// the diagonal of `noise` (:21-27)
LVI_MARG_HD void noise_diag(double acc_n, double gyr_n, double acc_w, double gyr_w, double* q)
{
    for (int k = 0; k < 3; k++) {
        q[k] = acc_n * acc_n; q[3 + k] = gyr_n * gyr_n; q[6 + k] = acc_n * acc_n; q[9 + k] = gyr_n * gyr_n;
        q[12 + k] = acc_w * acc_w; q[15 + k] = gyr_w * gyr_w;
    }
}

// the constructor (:13-18) without its matrices
LVI_MARG_HD void state_reset(State& s, const double* acc_0, const double* gyr_0, const double* ba, const double* bg)
{
    s.sum_dt = 0.;
    for (int k = 0; k < 3; k++) {
        s.delta_p[k] = 0.; s.delta_v[k] = 0.; s.delta_q[k] = 0.;
        s.linearized_ba[k] = ba[k]; s.linearized_bg[k] = bg[k]; s.acc_0[k] = acc_0[k]; s.gyr_0[k] = gyr_0[k];
    }
    s.delta_q[3] = 1.;
}
LVI_MARG_HD void matrices_reset(double* jacobian, double* covariance)
{
    for (int k = 0; k < N * N; k++) { jacobian[k] = (k / N == k % N) ? 1. : 0.; covariance[k] = 0.; }
}

// :63-71 and :148-156: the vector chain of one propagate; g receives what F and V of this step are built from
LVI_MARG_HD void step_state(State& s, double dt, const double* acc_1, const double* gyr_1, StepGeom& g)
{
    g.dt = dt;
    for (int k = 0; k < 3; k++) {
        g.a0[k] = s.acc_0[k] - s.linearized_ba[k];
        g.a1[k] = acc_1[k] - s.linearized_ba[k];
        g.w[k] = 0.5 * (s.gyr_0[k] + gyr_1[k]) - s.linearized_bg[k];
    }
    quat_to_rot(s.delta_q, g.R0);
    double un_acc_0[3], un_acc_1[3], rq[4];
    mat3_vec(g.R0, g.a0, un_acc_0);
    const double dq[4] = {g.w[0] * dt / 2, g.w[1] * dt / 2, g.w[2] * dt / 2, 1.0};
    quat_mul(s.delta_q, dq, rq);
    quat_to_rot(rq, g.R1);
    mat3_vec(g.R1, g.a1, un_acc_1);
    for (int k = 0; k < 3; k++) {
        const double un_acc = 0.5 * (un_acc_0[k] + un_acc_1[k]);
        s.delta_p[k] = s.delta_p[k] + s.delta_v[k] * dt + 0.5 * un_acc * dt * dt;
        s.delta_v[k] = s.delta_v[k] + un_acc * dt;
    }
    const double n = std::sqrt(rq[0] * rq[0] + rq[1] * rq[1] + rq[2] * rq[2] + rq[3] * rq[3]);
    for (int k = 0; k < 4; k++) s.delta_q[k] = rq[k] / n;
    s.sum_dt = s.sum_dt + dt;
    for (int k = 0; k < 3; k++) { s.acc_0[k] = acc_1[k]; s.gyr_0[k] = gyr_1[k]; }
}

// :90-120: the entries (i, j) of every 3 x 3 block of F and V, and for i == j the entries of the diagonal blocks
LVI_MARG_HD void build_entry(const StepGeom& g, int i, int j, double* F, double* V)
{
    const double dt = g.dt;
    const double *R0 = g.R0 + 3 * i, *R1 = g.R1 + 3 * i;             // row i
    double A0[9], A1[9], W[9];
    skew(g.a0, A0); skew(g.a1, A1); skew(g.w, W);
    double K[3];                                                      // column j of I - R_w_x dt
    for (int k = 0; k < 3; k++) K[k] = (k == j ? 1.0 : 0.0) - W[3 * k + j] * dt;
    double x1q[3], x1h[3];                                            // row i of (-0.25 R1) A1 and of (-0.5 R1) A1
    for (int k = 0; k < 3; k++) {
        x1q[k] = (-0.25 * R1[0]) * A1[k] + (-0.25 * R1[1]) * A1[3 + k] + (-0.25 * R1[2]) * A1[6 + k];
        x1h[k] = (-0.5 * R1[0]) * A1[k] + (-0.5 * R1[1]) * A1[3 + k] + (-0.5 * R1[2]) * A1[6 + k];
    }
    const double x0q = (-0.25 * R0[0]) * A0[j] + (-0.25 * R0[1]) * A0[3 + j] + (-0.25 * R0[2]) * A0[6 + j];
    const double x0h = (-0.5 * R0[0]) * A0[j] + (-0.5 * R0[1]) * A0[3 + j] + (-0.5 * R0[2]) * A0[6 + j];
    const double x1qK = x1q[0] * K[0] + x1q[1] * K[1] + x1q[2] * K[2];
    const double x1hK = x1h[0] * K[0] + x1h[1] * K[1] + x1h[2] * K[2];
    F[N * i + 3 + j] = x0q * dt * dt + x1qK * dt * dt;
    F[N * i + 9 + j] = (-0.25 * (R0[j] + R1[j])) * dt * dt;
    F[N * i + 12 + j] = x1q[j] * dt * dt * -dt;
    F[N * (3 + i) + 3 + j] = K[i];
    F[N * (6 + i) + 3 + j] = x0h * dt + x1hK * dt;
    F[N * (6 + i) + 9 + j] = (-0.5 * (R0[j] + R1[j])) * dt;
    F[N * (6 + i) + 12 + j] = x1h[j] * dt * -dt;
    // 0.25 * -R1 * A1 and 0.5 * -R1 * A1
    const double y1q = (0.25 * -R1[0]) * A1[j] + (0.25 * -R1[1]) * A1[3 + j] + (0.25 * -R1[2]) * A1[6 + j];
    const double y1h = (0.5 * -R1[0]) * A1[j] + (0.5 * -R1[1]) * A1[3 + j] + (0.5 * -R1[2]) * A1[6 + j];
    V[NV * i + j] = (0.25 * R0[j]) * dt * dt;
    V[NV * i + 3 + j] = y1q * dt * dt * 0.5 * dt;
    V[NV * i + 6 + j] = (0.25 * R1[j]) * dt * dt;
    V[NV * i + 9 + j] = V[NV * i + 3 + j];
    V[NV * (6 + i) + j] = (0.5 * R0[j]) * dt;
    V[NV * (6 + i) + 3 + j] = y1h * dt * 0.5 * dt;
    V[NV * (6 + i) + 6 + j] = (0.5 * R1[j]) * dt;
    V[NV * (6 + i) + 9 + j] = V[NV * (6 + i) + 3 + j];
    if (i == j) {
        F[N * i + i] = 1.0; F[N * i + 6 + i] = dt;
        F[N * (3 + i) + 12 + i] = -1.0 * dt;
        F[N * (6 + i) + 6 + i] = 1.0; F[N * (9 + i) + 9 + i] = 1.0; F[N * (12 + i) + 12 + i] = 1.0;
        V[NV * (3 + i) + 3 + i] = 0.5 * dt; V[NV * (3 + i) + 9 + i] = 0.5 * dt;
        V[NV * (9 + i) + 12 + i] = dt; V[NV * (12 + i) + 15 + i] = dt;
    }
}

// (F X)(r, c), X row-major N x N
LVI_MARG_HD double f_dot(const double* F, int r, const double* X, int c)
{
    const unsigned m = fmask(r);
    double s = 0.;
    for (int k = 0; k < N; k++)
        if ((m >> k) & 1u) s = s + F[N * r + k] * X[N * k + c];
    return s;
}
// (T F')(r, c)
LVI_MARG_HD double tf_dot(const double* T, int r, const double* F, int c)
{
    const unsigned m = fmask(c);
    double s = 0.;
    for (int k = 0; k < N; k++)
        if ((m >> k) & 1u) s = s + T[N * r + k] * F[N * c + k];
    return s;
}
// (V noise V')(r, c)
LVI_MARG_HD double vqv_dot(const double* V, const double* q, int r, int c)
{
    const unsigned m = vmask(r) & vmask(c);
    double s = 0.;
    for (int k = 0; k < NV; k++)
        if ((m >> k) & 1u) s = s + (V[NV * r + k] * q[k]) * V[NV * c + k];
    return s;
}

// :124-125 on the host: work holds F (225), V (270), T (225) and the new jacobian (225)
LVI_MARG_HD void step_matrices(const StepGeom& g, const double* q, double* jacobian, double* covariance, double* work)
{
    double *F = work, *V = work + 225, *T = work + 495, *Jn = work + 720;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) build_entry(g, i, j, F, V);
    for (int r = 0; r < N; r++)
        for (int c = 0; c < N; c++) { Jn[N * r + c] = f_dot(F, r, jacobian, c); T[N * r + c] = f_dot(F, r, covariance, c); }
    for (int r = 0; r < N; r++)
        for (int c = 0; c < N; c++) { jacobian[N * r + c] = Jn[N * r + c]; covariance[N * r + c] = tf_dot(T, r, F, c) + vqv_dot(V, q, r, c); }
}
constexpr int WORK_DOUBLES = 945;

// push_back of n samples (dt [n], acc [n][3], gyr [n][3]) onto a state and its matrices
LVI_MARG_HD void integrate(State& s, double* jacobian, double* covariance, const double* q, int n, const double* dt, const double* acc, const double* gyr,
                           double* work)
{
    StepGeom g;
    for (int k = 0; k < n; k++) {
        step_state(s, dt[k], acc + 3 * k, gyr + 3 * k, g);
        step_matrices(g, q, jacobian, covariance, work);
    }
}

// estimator.cpp:105-112 with acc_0, gyr_0 the estimator's: Rs[j] *= deltaQ(un_gyr dt).toRotationMatrix() with the
// quaternion (1, theta / 2) as it stands, then Ps, then Vs
LVI_MARG_HD void nav_step(Nav& n, const double* acc_0, const double* gyr_0, double dt, const double* acc, const double* gyr, const double* G)
{
    double a[3], un_acc_0[3], un_acc_1[3], th[3], dR[9], Rn[9];
    for (int k = 0; k < 3; k++) a[k] = acc_0[k] - n.Ba[k];
    mat3_vec(n.R, a, un_acc_0);
    for (int k = 0; k < 3; k++) {
        un_acc_0[k] = un_acc_0[k] - G[k];
        th[k] = (0.5 * (gyr_0[k] + gyr[k]) - n.Bg[k]) * dt;
    }
    const double dq[4] = {th[0] / 2.0, th[1] / 2.0, th[2] / 2.0, 1.0};
    quat_to_rot(dq, dR);
    mat3_mul(n.R, dR, Rn);
    for (int k = 0; k < 9; k++) n.R[k] = Rn[k];
    for (int k = 0; k < 3; k++) a[k] = acc[k] - n.Ba[k];
    mat3_vec(n.R, a, un_acc_1);
    for (int k = 0; k < 3; k++) {
        const double un_acc = 0.5 * (un_acc_0[k] + (un_acc_1[k] - G[k]));
        n.P[k] = n.P[k] + (dt * n.V[k] + 0.5 * dt * dt * un_acc);
        n.V[k] = n.V[k] + dt * un_acc;
    }
}

}  // namespace lvi_preint_math
