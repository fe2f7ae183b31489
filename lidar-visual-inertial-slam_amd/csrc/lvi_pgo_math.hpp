// SE(3) pieces of the pose-graph optimiser (include/lvi_pgo.h), usable from host and device: Expmap, Logmap,
// their derivatives, the adjoint and the errors and Jacobians of the prior and between factors.  All double.  The
// conventions restate GTSAM's Pose3 from memory (GTSAM is not vendored): tangent order rotation then translation,
// right perturbations X <- X * Retract(delta), factor error = Local(measured, h(x)), and
//   full_logmap = 1: Local = Pose3::Logmap, Retract = Pose3::Expmap (GTSAM_POSE3_EXPMAP)
//   full_logmap = 0: Local = [Rot3::Logmap(R); t], Retract = (Rot3::Expmap(w), v)   (the first-order chart)
// tests/pgo_ref.py states the same formulas in numpy, with the same series switches, and checks its Jacobians against
// central differences; the CPU tier compiles this header alone and compares the two.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define LVI_PGO_HD __host__ __device__ inline
#else
#define LVI_PGO_HD inline
#endif

namespace lvi_pgo_math {

struct Pose { double R[9]; double t[3]; };             // R row-major

constexpr double PGO_SERIES_TH2 = 0.04;               // below theta^2 = 0.04 the coefficients come from their Taylor series

// a = sin(th)/th, b = (1 - cos th)/th^2, c = (th - sin th)/th^3
LVI_PGO_HD void so3_abc(double th2, double* a, double* b, double* c)
{
    if (th2 < PGO_SERIES_TH2) {
        *a = 1. - th2 / 6. * (1. - th2 / 20. * (1. - th2 / 42. * (1. - th2 / 72. * (1. - th2 / 110.))));
        *b = .5 - th2 / 24. * (1. - th2 / 30. * (1. - th2 / 56. * (1. - th2 / 90. * (1. - th2 / 132.))));
        *c = 1. / 6. - th2 / 120. * (1. - th2 / 42. * (1. - th2 / 72. * (1. - th2 / 110. * (1. - th2 / 156.))));
    } else {
        const double th = std::sqrt(th2), s = std::sin(th), co = std::cos(th);
        *a = s / th; *b = (1. - co) / th2; *c = (th - s) / (th2 * th);
    }
}
// g of Jr^-1(w) = I + W/2 + g W^2 (and Jl^-1 = I - W/2 + g W^2): g = (1 - a / (2 b)) / th^2
LVI_PGO_HD double so3_g(double th2)
{
    if (th2 < PGO_SERIES_TH2)
        return 1. / 12. + th2 * (1. / 720. + th2 * (1. / 30240. + th2 * (1. / 1209600. + th2 * (1. / 47900160. + th2 * (691. / 1307674368000.)))));
    double a, b, c;
    so3_abc(th2, &a, &b, &c);
    return (1. - a / (2. * b)) / th2;
}
// d = (th^2 + 2 cos th - 2) / (2 th^4), e = (2 th - 3 sin th + th cos th) / (2 th^5): the last two coefficients of Q below
LVI_PGO_HD void se3_de(double th2, double* d, double* e)
{
    if (th2 < PGO_SERIES_TH2) {
        *d = 1. / 24. - th2 / 720. * (1. - th2 / 56. * (1. - th2 / 90. * (1. - th2 / 132. * (1. - th2 / 182.))));
        *e = 1. / 120. + th2 * (-2. / 5040. + th2 * (3. / 362880. + th2 * (-4. / 39916800. + th2 * (5. / 6227020800. + th2 * (-6. / 1307674368000.)))));
    } else {
        const double th = std::sqrt(th2), s = std::sin(th), co = std::cos(th), th4 = th2 * th2;
        *d = (th2 + 2. * co - 2.) / (2. * th4);
        *e = (2. * th - 3. * s + th * co) / (2. * th4 * th);
    }
}

LVI_PGO_HD void hat(const double w[3], double W[9])
{
    W[0] = 0.; W[1] = -w[2]; W[2] = w[1]; W[3] = w[2]; W[4] = 0.; W[5] = -w[0]; W[6] = -w[1]; W[7] = w[0]; W[8] = 0.;
}
LVI_PGO_HD void mat3_mul(const double A[9], const double B[9], double C[9])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
LVI_PGO_HD void mat3_vec(const double A[9], const double v[3], double o[3])
{
    for (int i = 0; i < 3; i++) o[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
}
// I * s0 + W * s1 + W^2 * s2
LVI_PGO_HD void poly_w(const double w[3], double s0, double s1, double s2, double M[9])
{
    double W[9], W2[9];
    hat(w, W);
    mat3_mul(W, W, W2);
    for (int i = 0; i < 9; i++) M[i] = s1 * W[i] + s2 * W2[i];
    M[0] += s0; M[4] += s0; M[8] += s0;
}

// Rot3::Expmap
LVI_PGO_HD void so3_exp(const double w[3], double R[9])
{
    double a, b, c;
    so3_abc(w[0] * w[0] + w[1] * w[1] + w[2] * w[2], &a, &b, &c);
    poly_w(w, 1., a, b, R);
}
// Rot3::Logmap: theta = atan2(|vee(R - R')| / 2, (tr R - 1) / 2); near pi the axis comes from the symmetric part
LVI_PGO_HD void so3_log(const double R[9], double w[3])
{
    const double v[3] = {.5 * (R[7] - R[5]), .5 * (R[2] - R[6]), .5 * (R[3] - R[1])};       // sin(th) * axis
    const double s = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), co = .5 * (R[0] + R[4] + R[8] - 1.);
    const double th = std::atan2(s, co);
    if (co > -0.9) {
        double k;                                                                            // th / sin(th)
        if (th * th < PGO_SERIES_TH2) { double a, b, c; so3_abc(th * th, &a, &b, &c); k = 1. / a; }
        else k = th / s;
        for (int i = 0; i < 3; i++) w[i] = k * v[i];
        return;
    }
    // (R + R') / 2 = cos I + (1 - cos) a a'
    int k = 0;
    if (R[4] > R[0]) k = 1;
    if (R[8] > R[4 * k]) k = 2;
    double ax[3];
    const double ak = std::sqrt((R[4 * k] - co) / (1. - co));
    for (int j = 0; j < 3; j++) ax[j] = j == k ? ak : .5 * (R[3 * k + j] + R[3 * j + k]) / ((1. - co) * ak);
    const double n = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    const double sg = (ax[0] * v[0] + ax[1] * v[1] + ax[2] * v[2]) < 0. ? -1. : 1.;
    for (int j = 0; j < 3; j++) w[j] = sg * th * ax[j] / n;
}
// d Logmap(R Exp(dw)) / d dw at 0 = Jr^-1(w)
LVI_PGO_HD void so3_jr_inv(const double w[3], double J[9])
{
    poly_w(w, 1., .5, so3_g(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), J);
}

// Retract at the origin: xi = (w, v)
LVI_PGO_HD void pose_exp(const double xi[6], int full, Pose* T)
{
    so3_exp(xi, T->R);
    if (full) {
        double a, b, c, V[9];
        so3_abc(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2], &a, &b, &c);
        poly_w(xi, 1., b, c, V);                                                             // Jl(w)
        mat3_vec(V, xi + 3, T->t);
    } else {
        for (int i = 0; i < 3; i++) T->t[i] = xi[3 + i];
    }
}
// Local at the origin
LVI_PGO_HD void pose_log(const Pose& T, int full, double xi[6])
{
    so3_log(T.R, xi);
    if (full) {
        double Vi[9];
        poly_w(xi, 1., -.5, so3_g(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]), Vi);      // Jl^-1(w)
        mat3_vec(Vi, T.t, xi + 3);
    } else {
        for (int i = 0; i < 3; i++) xi[3 + i] = T.t[i];
    }
}
LVI_PGO_HD void pose_mul(const Pose& A, const Pose& B, Pose* C)
{
    Pose o;
    mat3_mul(A.R, B.R, o.R);
    mat3_vec(A.R, B.t, o.t);
    for (int i = 0; i < 3; i++) o.t[i] += A.t[i];
    *C = o;
}
LVI_PGO_HD void pose_inv(const Pose& A, Pose* B)
{
    Pose o;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) o.R[3 * i + j] = A.R[3 * j + i];
    mat3_vec(o.R, A.t, o.t);
    for (int i = 0; i < 3; i++) o.t[i] = -o.t[i];
    *B = o;
}
// Pose3::AdjointMap: [R 0; [t]x R, R], 6x6 row-major
LVI_PGO_HD void pose_adjoint(const Pose& T, double Ad[36])
{
    double Tx[9], TR[9];
    hat(T.t, Tx);
    mat3_mul(Tx, T.R, TR);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            Ad[6 * i + j] = T.R[3 * i + j]; Ad[6 * i + 3 + j] = 0.;
            Ad[6 * (3 + i) + j] = TR[3 * i + j]; Ad[6 * (3 + i) + 3 + j] = T.R[3 * i + j];
        }
}
// the coupling block of the SE(3) left Jacobian for xi = (phi, rho) (Barfoot, State Estimation for Robotics, eq. 7.86b)
LVI_PGO_HD void se3_q(const double phi[3], const double rho[3], double Q[9])
{
    const double th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
    double a, b, c, d, e, P[9], R[9], PR[9], RP[9], PRP[9], PPR[9], RPP[9], PRPP[9], PPRP[9];
    so3_abc(th2, &a, &b, &c);
    se3_de(th2, &d, &e);
    hat(phi, P); hat(rho, R);
    mat3_mul(P, R, PR); mat3_mul(R, P, RP); mat3_mul(PR, P, PRP);
    mat3_mul(P, PR, PPR); mat3_mul(RP, P, RPP); mat3_mul(PRP, P, PRPP); mat3_mul(P, PRP, PPRP);
    for (int i = 0; i < 9; i++)
        Q[i] = .5 * R[i] + c * (PR[i] + RP[i] + PRP[i]) + d * (PPR[i] + RPP[i] - 3. * PRP[i]) + e * (PRPP[i] + PPRP[i]);
}
// d Local(E * Retract(delta)) / d delta at 0, for xi = Local(E): 6x6 row-major
//   full: Jr^-1(xi) = [Jr^-1(w) 0; -Jr^-1(w) Qr Jr^-1(w), Jr^-1(w)], Qr = Q(-w, -u)      chart: [Jr^-1(w) 0; 0 R_E]
LVI_PGO_HD void pose_local_jac(const Pose& E, const double xi[6], int full, double J[36])
{
    double Ji[9];
    so3_jr_inv(xi, Ji);
    for (int i = 0; i < 36; i++) J[i] = 0.;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) J[6 * i + j] = Ji[3 * i + j];
    if (full) {
        const double nw[3] = {-xi[0], -xi[1], -xi[2]}, nu[3] = {-xi[3], -xi[4], -xi[5]};
        double Q[9], JQ[9], JQJ[9];
        se3_q(nw, nu, Q);
        mat3_mul(Ji, Q, JQ);
        mat3_mul(JQ, Ji, JQJ);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) { J[6 * (3 + i) + j] = -JQJ[3 * i + j]; J[6 * (3 + i) + 3 + j] = Ji[3 * i + j]; }
    } else {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) J[6 * (3 + i) + 3 + j] = E.R[3 * i + j];
    }
}
LVI_PGO_HD void mat6_mul(const double A[36], const double B[36], double C[36])
{
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            double s = 0.;
            for (int k = 0; k < 6; k++) s += A[6 * i + k] * B[6 * k + j];
            C[6 * i + j] = s;
        }
}
// PriorFactor: r = Local(Z^-1 X), B = d r / d delta_X
LVI_PGO_HD void prior_error(const Pose& X, const Pose& Z, int full, double r[6], double B[36])
{
    Pose Zi, E;
    pose_inv(Z, &Zi);
    pose_mul(Zi, X, &E);
    pose_log(E, full, r);
    pose_local_jac(E, r, full, B);
}
// BetweenFactor(i, j, Z): r = Local(Z^-1 Xi^-1 Xj), A = d r / d delta_i = -B Ad(h^-1), B = d r / d delta_j, h = Xi^-1 Xj
LVI_PGO_HD void between_error(const Pose& Xi, const Pose& Xj, const Pose& Z, int full, double r[6], double A[36], double B[36])
{
    Pose Xii, h, hi, Zi, E;
    pose_inv(Xi, &Xii);
    pose_mul(Xii, Xj, &h);
    pose_inv(Z, &Zi);
    pose_mul(Zi, h, &E);
    pose_log(E, full, r);
    pose_local_jac(E, r, full, B);
    pose_inv(h, &hi);
    double Ad[36];
    pose_adjoint(hi, Ad);
    mat6_mul(B, Ad, A);
    for (int i = 0; i < 36; i++) A[i] = -A[i];
}
// GPSFactor(key, z) (include/lvi_pgo_gps.h): r = X.translation() - z; J = d r / d delta_X = [0 | R], 3x6 row-major, in both
// charts (the translation of X * Retract(delta) is t + R v + O(|delta|^2) whichever chart Retract is)
LVI_PGO_HD void gps_error(const Pose& X, const double z[3], double r[3], double J[18])
{
    for (int i = 0; i < 3; i++) {
        r[i] = X.t[i] - z[i];
        for (int j = 0; j < 3; j++) { J[6 * i + j] = 0.; J[6 * i + 3 + j] = X.R[3 * i + j]; }
    }
}
// X <- X * Retract(delta)
LVI_PGO_HD void pose_retract(Pose* X, const double delta[6], int full)
{
    Pose D;
    pose_exp(delta, full, &D);
    pose_mul(*X, D, X);
}

// gtsam::Pose3(Rot3::RzRyRx(roll, pitch, yaw), Point3(x, y, z)) from the float pose (roll, pitch, yaw, x, y, z): the
// arithmetic of pose3Matrix in host/lvi_loop_host.hpp
LVI_PGO_HD void pose_from_rpyxyz(const float p[6], Pose* T)
{
    const double roll = p[0], pitch = p[1], yaw = p[2];
    const double A = std::cos(yaw), B = std::sin(yaw), C = std::cos(pitch), D = std::sin(pitch), E = std::cos(roll), F = std::sin(roll);
    const double R[9] = {A * C, A * D * F - B * E, B * F + A * D * E, B * C, A * E + B * D * F, B * D * E - A * F, -D, C * F, C * E};
    for (int i = 0; i < 9; i++) T->R[i] = R[i];
    for (int i = 0; i < 3; i++) T->t[i] = p[3 + i];
}
// Rot3::rpy and the translation, cast to float
LVI_PGO_HD void pose_to_rpyxyz(const Pose& T, float p[6])
{
    p[0] = (float)std::atan2(T.R[7], T.R[8]);
    p[1] = (float)std::atan2(-T.R[6], std::hypot(T.R[7], T.R[8]));
    p[2] = (float)std::atan2(T.R[3], T.R[0]);
    for (int i = 0; i < 3; i++) p[3 + i] = (float)T.t[i];
}
LVI_PGO_HD void pose_from_matrix(const double M[16], Pose* T)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T->R[3 * i + j] = M[4 * i + j];
        T->t[i] = M[4 * i + 3];
    }
}
LVI_PGO_HD void pose_to_matrix(const Pose& T, double M[16])
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) M[4 * i + j] = T.R[3 * i + j];
        M[4 * i + 3] = T.t[i];
        M[12 + i] = 0.;
    }
    M[15] = 1.;
}

// 6x6 SPD: lower Cholesky factor (row-major, upper part untouched) and the solve L L' x = b in place
LVI_PGO_HD void chol6(const double A[36], double L[36])
{
    for (int j = 0; j < 6; j++) {
        double s = A[6 * j + j];
        for (int k = 0; k < j; k++) s -= L[6 * j + k] * L[6 * j + k];
        const double d = std::sqrt(s);
        L[6 * j + j] = d;
        for (int i = j + 1; i < 6; i++) {
            double t = A[6 * i + j];
            for (int k = 0; k < j; k++) t -= L[6 * i + k] * L[6 * j + k];
            L[6 * i + j] = t / d;
        }
    }
}
LVI_PGO_HD void chol6_solve(const double L[36], double b[6])
{
    for (int i = 0; i < 6; i++) {
        double s = b[i];
        for (int k = 0; k < i; k++) s -= L[6 * i + k] * b[k];
        b[i] = s / L[6 * i + i];
    }
    for (int i = 5; i >= 0; i--) {
        double s = b[i];
        for (int k = i + 1; k < 6; k++) s -= L[6 * k + i] * b[k];
        b[i] = s / L[6 * i + i];
    }
}
// general 6x6 solve A x = b by elimination with partial pivoting (A and b are overwritten; x in b)
LVI_PGO_HD void solve6(double A[36], double b[6])
{
    for (int j = 0; j < 6; j++) {
        int p = j;
        for (int i = j + 1; i < 6; i++) if (std::fabs(A[6 * i + j]) > std::fabs(A[6 * p + j])) p = i;
        if (p != j) {
            for (int k = 0; k < 6; k++) { const double t = A[6 * j + k]; A[6 * j + k] = A[6 * p + k]; A[6 * p + k] = t; }
            const double t = b[j]; b[j] = b[p]; b[p] = t;
        }
        for (int i = j + 1; i < 6; i++) {
            const double f = A[6 * i + j] / A[6 * j + j];
            for (int k = j; k < 6; k++) A[6 * i + k] -= f * A[6 * j + k];
            b[i] -= f * b[j];
        }
    }
    for (int i = 5; i >= 0; i--) {
        double s = b[i];
        for (int k = i + 1; k < 6; k++) s -= A[6 * i + k] * b[k];
        b[i] = s / A[6 * i + i];
    }
}

}  // namespace lvi_pgo_math
