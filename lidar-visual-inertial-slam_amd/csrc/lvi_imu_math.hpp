// IMUFactor of the sliding-window solve (include/lvi_win.h), usable from host and device and compilable
// without HIP: IntegrationBase::evaluate (integration_base.h:160-186), IMUFactor::Evaluate (imu_factor.h:18-178) with the
// #else branches the reference compiles (:96-97, :124, :150-151) and sqrt_info = LLT(covariance^-1).matrixL()' (:63).
// All double.  Quaternions are x y z w; vectors are rotated by the rotation matrix of the quaternion taken as unit, as
// Eigen's q * v does; Quaternion::inverse() is conjugate / squaredNorm, as Eigen's.  The Jacobian has the local columns:
// pose_i 0..5, speed_bias_i 6..14, pose_j 15..20, speed_bias_j 21..29 (the seventh column of a pose is zero and never
// stored).  Rows: O_P 0, O_R 3, O_V 6, O_BA 9, O_BG 12.  tests/win_ref.py states the same formulas in numpy and mpmath.
#pragma once
#include "lvi_marg_math.hpp"

namespace lvi_imu_math {

using lvi_marg_math::mat3_tvec;
using lvi_marg_math::mat3_vec;
using lvi_marg_math::quat_to_rot;
using lvi_marg_math::skew;

constexpr int IMU_ROWS = 15, IMU_COLS = 30;
constexpr int O_P = 0, O_R = 3, O_V = 6, O_BA = 9, O_BG = 12;
constexpr int C_POSE_I = 0, C_SB_I = 6, C_POSE_J = 15, C_SB_J = 21;

struct ImuPre {
    double sum_dt, delta_p[3], delta_q[4], delta_v[3], linearized_ba[3], linearized_bg[3], jacobian[225];
};

LVI_MARG_HD void quat_mul(const double* a, const double* b, double* o)      // Hamilton product, x y z w
{
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    o[0] = aw * bx + ax * bw + ay * bz - az * by;
    o[1] = aw * by + ay * bw + az * bx - ax * bz;
    o[2] = aw * bz + az * bw + ax * by - ay * bx;
    o[3] = aw * bw - ax * bx - ay * by - az * bz;
}
LVI_MARG_HD void quat_inv(const double* q, double* o)
{
    const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    o[0] = -q[0] / n2; o[1] = -q[1] / n2; o[2] = -q[2] / n2; o[3] = q[3] / n2;
}
// bottomRightCorner<3, 3>() of Utility::Qleft(q) (utility.h:51-58): w I + skew(v)
LVI_MARG_HD void qleft_br(const double* q, double* M)
{
    skew(q, M);
    M[0] += q[3]; M[4] += q[3]; M[8] += q[3];
}
// ... of Qleft(a) * Qright(b) (:61-68): -a_v b_v' + (a_w I + skew(a_v)) (b_w I - skew(b_v))
LVI_MARG_HD void qleft_qright_br(const double* a, const double* b, double* M)
{
    double L[9], R[9];
    qleft_br(a, L);
    skew(b, R);
    for (int k = 0; k < 9; k++) R[k] = -R[k];
    R[0] += b[3]; R[4] += b[3]; R[8] += b[3];
    lvi_marg_math::mat3_mul(L, R, M);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[3 * i + j] += -a[i] * b[j];
}

// lower Cholesky factor of the symmetric n x n matrix A (row-major, its lower triangle is read) into L; false on a pivot
// that is not positive
LVI_MARG_HD bool chol_lower(int n, const double* A, double* L)
{
    for (int k = 0; k < n * n; k++) L[k] = 0.;
    for (int j = 0; j < n; j++) {
        double d = A[n * j + j];
        for (int k = 0; k < j; k++) d -= L[n * j + k] * L[n * j + k];
        if (!(d > 0.)) return false;
        const double s = std::sqrt(d);
        L[n * j + j] = s;
        for (int i = j + 1; i < n; i++) {
            double v = A[n * i + j];
            for (int k = 0; k < j; k++) v -= L[n * i + k] * L[n * j + k];
            L[n * i + j] = v / s;
        }
    }
    return true;
}

// imu_factor.h:63: covariance = C C', covariance^-1 = C^-T C^-1, its LLT factor L, sqrt_info = L'.  work: 3 x 225 doubles.
LVI_MARG_HD bool imu_sqrt_info(const double* cov, double* sqrt_info, double* work)
{
    constexpr int n = IMU_ROWS;
    double *C = work, *Ci = work + 225, *Inf = work + 450;
    if (!chol_lower(n, cov, C)) return false;
    for (int k = 0; k < n * n; k++) Ci[k] = 0.;
    for (int j = 0; j < n; j++) {                          // columns of C^-1 by forward substitution
        Ci[n * j + j] = 1. / C[n * j + j];
        for (int i = j + 1; i < n; i++) {
            double v = 0.;
            for (int k = j; k < i; k++) v -= C[n * i + k] * Ci[n * k + j];
            Ci[n * i + j] = v / C[n * i + i];
        }
    }
    for (int i = 0; i < n; i++)
        for (int j = 0; j <= i; j++) {
            double v = 0.;
            for (int k = i; k < n; k++) v += Ci[n * k + i] * Ci[n * k + j];
            Inf[n * i + j] = v; Inf[n * j + i] = v;
        }
    if (!chol_lower(n, Inf, C)) return false;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) sqrt_info[n * i + j] = C[n * j + i];
    return true;
}

// residual [15] and, when J is not null, the Jacobian row-major [15][30], both before the multiplication by sqrt_info
LVI_MARG_HD void imu_eval_raw(const double* pose_i, const double* sb_i, const double* pose_j, const double* sb_j, const ImuPre& p, const double* G,
                              double* r, double* J)
{
    const double *Pi = pose_i, *Qi = pose_i + 3, *Vi = sb_i, *Bai = sb_i + 3, *Bgi = sb_i + 6;
    const double *Pj = pose_j, *Qj = pose_j + 3, *Vj = sb_j, *Baj = sb_j + 3, *Bgj = sb_j + 6;
    const double dt = p.sum_dt;
    double Ri[9];
    quat_to_rot(Qi, Ri);
    double dba[3], dbg[3], th[3];
    for (int k = 0; k < 3; k++) { dba[k] = Bai[k] - p.linearized_ba[k]; dbg[k] = Bgi[k] - p.linearized_bg[k]; }
    const auto jb = [&](int row, int col, const double* v, double* o) {       // jacobian.block<3, 3>(row, col) v
        for (int i = 0; i < 3; i++) o[i] = p.jacobian[15 * (row + i) + col] * v[0] + p.jacobian[15 * (row + i) + col + 1] * v[1] + p.jacobian[15 * (row + i) + col + 2] * v[2];
    };
    jb(O_R, O_BG, dbg, th);
    const double dq[4] = {th[0] / 2.0, th[1] / 2.0, th[2] / 2.0, 1.0};      // Utility::deltaQ
    double cdq[4], cdv[3], cdp[3], a[3], b[3];
    quat_mul(p.delta_q, dq, cdq);
    jb(O_V, O_BA, dba, a); jb(O_V, O_BG, dbg, b);
    for (int k = 0; k < 3; k++) cdv[k] = p.delta_v[k] + a[k] + b[k];
    jb(O_P, O_BA, dba, a); jb(O_P, O_BG, dbg, b);
    for (int k = 0; k < 3; k++) cdp[k] = p.delta_p[k] + a[k] + b[k];
    double up[3], uv[3], rp[3], rv[3];
    for (int k = 0; k < 3; k++) {
        up[k] = 0.5 * G[k] * dt * dt + Pj[k] - Pi[k] - Vi[k] * dt;
        uv[k] = G[k] * dt + Vj[k] - Vi[k];
    }
    mat3_tvec(Ri, up, rp); mat3_tvec(Ri, uv, rv);
    double Qi_inv[4], QiQj[4], cdq_inv[4], e[4];
    quat_inv(Qi, Qi_inv); quat_mul(Qi_inv, Qj, QiQj); quat_inv(cdq, cdq_inv); quat_mul(cdq_inv, QiQj, e);
    for (int k = 0; k < 3; k++) {
        r[O_P + k] = rp[k] - cdp[k];
        r[O_R + k] = 2.0 * e[k];
        r[O_V + k] = rv[k] - cdv[k];
        r[O_BA + k] = Baj[k] - Bai[k];
        r[O_BG + k] = Bgj[k] - Bgi[k];
    }
    if (!J) return;
    for (int k = 0; k < IMU_ROWS * IMU_COLS; k++) J[k] = 0.;
    const auto at = [&](int row, int col) -> double& { return J[IMU_COLS * row + col]; };
    double Sp[9], Sv[9], M[9], Qj_inv[4], QjQi[4], t4[4];
    skew(rp, Sp); skew(rv, Sv);
    quat_inv(Qj, Qj_inv); quat_mul(Qj_inv, Qi, QjQi);
    // pose_i (:85-110)
    qleft_qright_br(QjQi, cdq, M);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            at(O_P + i, C_POSE_I + j) = -Ri[3 * j + i];
            at(O_P + i, C_POSE_I + 3 + j) = Sp[3 * i + j];
            at(O_R + i, C_POSE_I + 3 + j) = -M[3 * i + j];
            at(O_V + i, C_POSE_I + 3 + j) = Sv[3 * i + j];
        }
    // speed_bias_i (:111-139)
    quat_mul(QjQi, p.delta_q, t4);
    qleft_br(t4, M);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            at(O_P + i, C_SB_I + j) = -Ri[3 * j + i] * dt;
            at(O_P + i, C_SB_I + 3 + j) = -p.jacobian[15 * (O_P + i) + O_BA + j];
            at(O_P + i, C_SB_I + 6 + j) = -p.jacobian[15 * (O_P + i) + O_BG + j];
            double s = 0.;
            for (int k = 0; k < 3; k++) s += M[3 * i + k] * p.jacobian[15 * (O_R + k) + O_BG + j];
            at(O_R + i, C_SB_I + 6 + j) = -s;
            at(O_V + i, C_SB_I + j) = -Ri[3 * j + i];
            at(O_V + i, C_SB_I + 3 + j) = -p.jacobian[15 * (O_V + i) + O_BA + j];
            at(O_V + i, C_SB_I + 6 + j) = -p.jacobian[15 * (O_V + i) + O_BG + j];
            at(O_BA + i, C_SB_I + 3 + j) = i == j ? -1. : 0.;
            at(O_BG + i, C_SB_I + 6 + j) = i == j ? -1. : 0.;
        }
    // pose_j (:140-158)
    quat_mul(cdq_inv, QiQj, t4);
    qleft_br(t4, M);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            at(O_P + i, C_POSE_J + j) = Ri[3 * j + i];
            at(O_R + i, C_POSE_J + 3 + j) = M[3 * i + j];
        }
    // speed_bias_j (:159-174)
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            at(O_V + i, C_SB_J + j) = Ri[3 * j + i];
            at(O_BA + i, C_SB_J + 3 + j) = i == j ? 1. : 0.;
            at(O_BG + i, C_SB_J + 6 + j) = i == j ? 1. : 0.;
        }
}

// out[i] = sum_k sqrt_info[i][k] v[k][col] over a row-major [15][ld] matrix: one entry of sqrt_info * (r or J)
LVI_MARG_HD double imu_info_dot(const double* sqrt_info, int i, const double* v, int ld, int col)
{
    double s = 0.;
    for (int k = 0; k < IMU_ROWS; k++) s += sqrt_info[IMU_ROWS * i + k] * v[ld * k + col];
    return s;
}

// PoseLocalParameterization::Plus (pose_local_parameterization.cpp:3-19)
LVI_MARG_HD void pose_plus(const double* x, const double* d, double* o)
{
    for (int k = 0; k < 3; k++) o[k] = x[k] + d[k];
    const double dq[4] = {d[3] / 2.0, d[4] / 2.0, d[5] / 2.0, 1.0};
    double q[4];
    quat_mul(x + 3, dq, q);
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 4; k++) o[3 + k] = q[k] / n;
}

}  // namespace lvi_imu_math
