// Factor evaluation of the sliding-window marginalisation (include/lvi_marg.h), usable from host and device and
// compilable without HIP: ProjectionFactor::Evaluate (projection_factor.cpp:21-121), ProjectionTdFactor::Evaluate
// (projection_td_factor.cpp:34-141), the loss correction of ResidualBlockInfo::Evaluate (marginalization_factor.cpp:37-68)
// with ceres' CauchyLoss and HuberLoss, and the dx of MarginalizationFactor::Evaluate (:344-362).  All double.
// A pose block is [p (3), q = x y z w (4)]; its Jacobian has the 6 local columns (the seventh is zero and never stored).
// Quaternions are taken as unit, as the reference's local parameterisation keeps them.  UNIT_SPHERE_ERROR is not defined
// in the reference (parameters.h:17) and is not restated.  tests/marg_ref.py states the same formulas in numpy and in
// mpmath; the CPU tier compiles this header alone and compares.
#pragma once
#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#define LVI_MARG_HD __host__ __device__ inline
#else
#define LVI_MARG_HD inline
#endif

namespace lvi_marg_math {

constexpr int PROJ_COLS = 20;        // pose_i 0..5, pose_j 6..11, extrinsic 12..17, inverse depth 18, td 19
constexpr int LOSS_NONE = 0, LOSS_CAUCHY = 1, LOSS_HUBER = 2;

// Eigen's Quaternion::toRotationMatrix, q = x y z w, R row-major
LVI_MARG_HD void quat_to_rot(const double* q, double* R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2. * x, ty = 2. * y, tz = 2. * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1. - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1. - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1. - (txx + tyy);
}
LVI_MARG_HD void mat3_mul(const double* A, const double* B, double* C)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
LVI_MARG_HD void mat3_tmul(const double* A, const double* B, double* C)      // A' B
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
LVI_MARG_HD void mat3_vec(const double* A, const double* v, double* o)
{
    for (int i = 0; i < 3; i++) o[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
}
LVI_MARG_HD void mat3_tvec(const double* A, const double* v, double* o)      // A' v
{
    for (int i = 0; i < 3; i++) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}
LVI_MARG_HD void skew(const double* v, double* S)
{
    S[0] = 0.; S[1] = -v[2]; S[2] = v[1];
    S[3] = v[2]; S[4] = 0.; S[5] = -v[0];
    S[6] = -v[1]; S[7] = v[0]; S[8] = 0.;
}

struct ProjObs {
    double pts_i[3], pts_j[3], vel_i[2], vel_j[2], td_i, td_j, row_i, row_j;   // rows: uv.y as observed
};
struct ProjConst { double sqrt_info, tr_over_row, half_row; };

// The two projection factors.  use_td 0: ProjectionFactor (td, velocities and rows unused, column 19 zero).
// r [2], J row-major [2][PROJ_COLS].
LVI_MARG_HD void projection_eval(const double* pose_i, const double* pose_j, const double* ex, double inv_dep_i, double td, int use_td,
                                 const ProjObs& o, const ProjConst& c, double* r, double* J)
{
    const double *Pi = pose_i, *Pj = pose_j, *tic = ex;
    double Ri[9], Rj[9], ric[9];
    quat_to_rot(pose_i + 3, Ri); quat_to_rot(pose_j + 3, Rj); quat_to_rot(ex + 3, ric);
    double pi_td[3] = {o.pts_i[0], o.pts_i[1], o.pts_i[2]}, pj_td[3] = {o.pts_j[0], o.pts_j[1], o.pts_j[2]};
    if (use_td) {
        const double ki = td - o.td_i + c.tr_over_row * (o.row_i - c.half_row), kj = td - o.td_j + c.tr_over_row * (o.row_j - c.half_row);
        pi_td[0] -= ki * o.vel_i[0]; pi_td[1] -= ki * o.vel_i[1];
        pj_td[0] -= kj * o.vel_j[0]; pj_td[1] -= kj * o.vel_j[1];
    }
    double pc_i[3], p_imu_i[3], p_w[3], d[3], p_imu_j[3], pc_j[3], t[3];
    for (int k = 0; k < 3; k++) pc_i[k] = pi_td[k] / inv_dep_i;
    mat3_vec(ric, pc_i, t);
    for (int k = 0; k < 3; k++) p_imu_i[k] = t[k] + tic[k];
    mat3_vec(Ri, p_imu_i, t);
    for (int k = 0; k < 3; k++) { p_w[k] = t[k] + Pi[k]; d[k] = p_w[k] - Pj[k]; }
    mat3_tvec(Rj, d, p_imu_j);
    for (int k = 0; k < 3; k++) d[k] = p_imu_j[k] - tic[k];
    mat3_tvec(ric, d, pc_j);
    const double dep_j = pc_j[2];
    r[0] = c.sqrt_info * (pc_j[0] / dep_j - pj_td[0]);
    r[1] = c.sqrt_info * (pc_j[1] / dep_j - pj_td[1]);

    double red[6] = {c.sqrt_info * (1. / dep_j), 0., c.sqrt_info * (-pc_j[0] / (dep_j * dep_j)),
                     0., c.sqrt_info * (1. / dep_j), c.sqrt_info * (-pc_j[1] / (dep_j * dep_j))};
    double M[9], N[9], Q[9], S[9], jac[18];
    // ric' Rj'
    double ricT_RjT[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) ricT_RjT[3 * i + j] = ric[i] * Rj[3 * j] + ric[3 + i] * Rj[3 * j + 1] + ric[6 + i] * Rj[3 * j + 2];
    mat3_mul(ricT_RjT, Ri, M);                                   // ric' Rj' Ri
    // pose_i: [ric' Rj', ric' Rj' Ri (-skew(pts_imu_i))]
    skew(p_imu_i, S);
    mat3_mul(M, S, N);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { jac[6 * i + j] = ricT_RjT[3 * i + j]; jac[6 * i + 3 + j] = -N[3 * i + j]; }
    for (int a = 0; a < 2; a++)
        for (int j = 0; j < 6; j++) J[PROJ_COLS * a + j] = red[3 * a] * jac[j] + red[3 * a + 1] * jac[6 + j] + red[3 * a + 2] * jac[12 + j];
    // pose_j: [-ric' Rj', ric' skew(pts_imu_j)]
    skew(p_imu_j, S);
    mat3_tmul(ric, S, N);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { jac[6 * i + j] = -ricT_RjT[3 * i + j]; jac[6 * i + 3 + j] = N[3 * i + j]; }
    for (int a = 0; a < 2; a++)
        for (int j = 0; j < 6; j++) J[PROJ_COLS * a + 6 + j] = red[3 * a] * jac[j] + red[3 * a + 1] * jac[6 + j] + red[3 * a + 2] * jac[12 + j];
    // extrinsic: [ric' (Rj' Ri - I), -tmp_r skew(pts_camera_i) + skew(tmp_r pts_camera_i) + skew(ric' (Rj' (Ri tic + Pi - Pj) - tic))]
    double RjT_Ri[9], tmp_r[9], v[3], u[3], S2[9], S3[9];
    mat3_tmul(Rj, Ri, RjT_Ri);
    for (int k = 0; k < 9; k++) Q[k] = RjT_Ri[k] - ((k % 4 == 0) ? 1. : 0.);
    mat3_tmul(ric, Q, N);                                        // ric' (Rj' Ri - I)
    mat3_mul(M, ric, tmp_r);
    skew(pc_i, S);
    mat3_mul(tmp_r, S, Q);
    mat3_vec(tmp_r, pc_i, v);
    skew(v, S2);
    mat3_vec(Ri, tic, v);
    for (int k = 0; k < 3; k++) v[k] = v[k] + Pi[k] - Pj[k];
    mat3_tvec(Rj, v, u);
    for (int k = 0; k < 3; k++) u[k] -= tic[k];
    mat3_tvec(ric, u, v);
    skew(v, S3);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { jac[6 * i + j] = N[3 * i + j]; jac[6 * i + 3 + j] = -Q[3 * i + j] + S2[3 * i + j] + S3[3 * i + j]; }
    for (int a = 0; a < 2; a++)
        for (int j = 0; j < 6; j++) J[PROJ_COLS * a + 12 + j] = red[3 * a] * jac[j] + red[3 * a + 1] * jac[6 + j] + red[3 * a + 2] * jac[12 + j];
    // inverse depth: reduce tmp_r pts_i_td * -1 / inv_dep^2
    mat3_vec(tmp_r, pi_td, v);
    for (int a = 0; a < 2; a++)
        J[PROJ_COLS * a + 18] = (red[3 * a] * v[0] + red[3 * a + 1] * v[1] + red[3 * a + 2] * v[2]) * -1.0 / (inv_dep_i * inv_dep_i);
    // td: reduce tmp_r velocity_i / inv_dep * -1 + sqrt_info velocity_j
    if (use_td) {
        const double vi[3] = {o.vel_i[0], o.vel_i[1], 0.};
        mat3_vec(tmp_r, vi, v);
        for (int a = 0; a < 2; a++)
            J[PROJ_COLS * a + 19] = (red[3 * a] * v[0] + red[3 * a + 1] * v[1] + red[3 * a + 2] * v[2]) / inv_dep_i * -1.0 + c.sqrt_info * o.vel_j[a];
    } else {
        J[19] = 0.; J[PROJ_COLS + 19] = 0.;
    }
}

// ceres::CauchyLoss(a) / ceres::HuberLoss(a)::Evaluate(s, rho); LOSS_NONE: the identity
LVI_MARG_HD void loss_rho(int type, double a, double s, double* rho)
{
    const double b = a * a;
    if (type == LOSS_CAUCHY) {
        const double c = 1. / b, sum = 1. + s * c, inv = 1. / sum;
        rho[0] = b * std::log(sum);
        rho[1] = inv > DBL_MIN ? inv : DBL_MIN;
        rho[2] = -c * (inv * inv);
    } else if (type == LOSS_HUBER && s > b) {
        const double rt = std::sqrt(s), q = a / rt;
        rho[0] = 2. * a * rt - b;
        rho[1] = q > DBL_MIN ? q : DBL_MIN;
        rho[2] = -rho[1] / (2. * s);
    } else {
        rho[0] = s; rho[1] = 1.; rho[2] = 0.;
    }
}

// marginalization_factor.cpp:37-68 as written, both branches, from rho[1] and rho[2]: r [n_res], J row-major [n_res][ld]
// of which n_cols columns are corrected
LVI_MARG_HD void loss_correct(int n_res, int n_cols, int ld, const double* rho, double* r, double* J)
{
    double sq_norm = 0.;
    for (int i = 0; i < n_res; i++) sq_norm += r[i] * r[i];
    const double sqrt_rho1 = std::sqrt(rho[1]);
    double residual_scaling, alpha_sq_norm;
    if (sq_norm == 0.0 || rho[2] <= 0.0) {
        residual_scaling = sqrt_rho1;
        alpha_sq_norm = 0.0;
    } else {
        const double D = 1.0 + 2.0 * sq_norm * rho[2] / rho[1];
        const double alpha = 1.0 - std::sqrt(D);
        residual_scaling = sqrt_rho1 / (1 - alpha);
        alpha_sq_norm = alpha / sq_norm;
    }
    for (int j = 0; j < n_cols; j++) {
        double rtJ = 0.;
        for (int i = 0; i < n_res; i++) rtJ += r[i] * J[ld * i + j];
        for (int i = 0; i < n_res; i++) J[ld * i + j] = sqrt_rho1 * (J[ld * i + j] - alpha_sq_norm * r[i] * rtJ);
    }
    for (int i = 0; i < n_res; i++) r[i] *= residual_scaling;
}

// the local size of a block: marginalization_factor.cpp:131-134
LVI_MARG_HD int local_size(int size) { return size == 7 ? 6 : size; }

// dx of one kept block (:349-361): x - x0, and for a size-7 block [dp, 2 (q0^-1 q).vec()] with the sign branch of :357-360
// (Utility::positify returns its argument unchanged, utility.h:41-48).  dx has local_size(size) entries.
LVI_MARG_HD void prior_dx(int size, const double* x, const double* x0, double* dx)
{
    if (size != 7) {
        for (int k = 0; k < size; k++) dx[k] = x[k] - x0[k];
        return;
    }
    for (int k = 0; k < 3; k++) dx[k] = x[k] - x0[k];
    // q0.inverse() = conjugate / squaredNorm
    const double n2 = x0[3] * x0[3] + x0[4] * x0[4] + x0[5] * x0[5] + x0[6] * x0[6];
    const double ax = -x0[3] / n2, ay = -x0[4] / n2, az = -x0[5] / n2, aw = x0[6] / n2;
    const double bx = x[3], by = x[4], bz = x[5], bw = x[6];
    const double w = aw * bw - ax * bx - ay * by - az * bz;
    const double vx = aw * bx + ax * bw + ay * bz - az * by;
    const double vy = aw * by + ay * bw + az * bx - ax * bz;
    const double vz = aw * bz + az * bw + ax * by - ay * bx;
    dx[3] = 2.0 * vx; dx[4] = 2.0 * vy; dx[5] = 2.0 * vz;
    if (!(w >= 0)) { dx[3] = 2.0 * -vx; dx[4] = 2.0 * -vy; dx[5] = 2.0 * -vz; }
}

// the symmetric Schur rotation that annihilates a_pq: J = [[c, s], [-s, c]], J' [[app, apq], [apq, aqq]] J diagonal
LVI_MARG_HD void jacobi_cs(double app, double aqq, double apq, double* c, double* s)
{
    const double tau = (aqq - app) / (2. * apq);
    const double t = (tau >= 0. ? 1. : -1.) / (std::fabs(tau) + std::sqrt(1. + tau * tau));
    *c = 1. / std::sqrt(1. + t * t);
    *s = t * *c;
}

}  // namespace lvi_marg_math
