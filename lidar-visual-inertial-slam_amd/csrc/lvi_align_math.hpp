// Visual-inertial alignment of vins_estimator's initialisation (include/lvi_align.h), usable from host and device
// and compilable without HIP: solveGyroscopeBias, TangentBasis, RefineGravity, LinearAlignment (initial/initial_aligment.cpp:
// 3-209), the excitation check (estimator.cpp:273-300) and the tail of visualInitialAlign with Utility::g2R (:450-486).  All
// double, built over lvi_preint_math.hpp (the repropagation is its step_state / build_entry / f_dot without the covariance).
// Quaternions are x y z w; matrices row-major.
//
// The order of every sum is part of the contract (tests/align_ref.py states the same operations term by term and the library
// is held to it bit for bit):
//   - a chain of scalars and matrices is evaluated left to right, as Eigen does: R_i' * dt * dt / 2 is ((R_i' dt) dt) / 2, a
//     3 x 3 product element is a b + c d + e f from the left, delta_p + R_i' R_j TIC - TIC is (delta_p + (R_i' R_j) TIC) - TIC;
//   - the identity factors of the reference (cov_inv, Matrix3d::Identity()) are exact and are left out;
//   - r_A = tmp_A' tmp_A and r_b = tmp_A' tmp_b are dense sums, started at 0, over the six rows in ascending order, zeros
//     of tmp_A included;
//   - every entry of A and b receives its pairs' contributions in ascending pair order, onto 0 (gyro, linear, the first
//     refinement) or onto the previous refinement's scaled system, which the reference does not clear; then the whole is
//     multiplied by 1000.0 entry by entry;
//   - the symmetric solve is this file's own: an unpivoted L D L' in natural order, every entry a left-looking dot product in
//     ascending k, (L[i][k] d[k]) L[j][k]; forward with ascending k, division by d, backward with ascending k.
//
// A system of F frames with a border of NB (4 linear, 3 refinement) has nd = 3 F diagonal unknowns and n = nd + NB.  It is
// block-tridiagonal with half bandwidth BAND = 5 plus the dense border, and the unpivoted factor has no fill outside that
// pattern, so it is stored and factored compactly: band[6 i + d] = A[i][i - d] (i < nd, d <= min(i, 5)) and
// bord[n k + j] = A[nd + k][j] (j <= nd + k).  A is symmetric bit for bit (products commute, sums share their order), so the
// lower triangle is the whole.  After the factorisation band[6 i] and bord[n k + nd + k] hold d, the rest L.
// A system with fewer equations than unknowns, 6 (F - 1) < n, is singular by count and is not factored: rounding may leave
// its zero pivot a tiny positive number.
#pragma once
#include "lvi_preint_math.hpp"

namespace lvi_align_math {

using lvi_imu_math::quat_inv;
using lvi_imu_math::quat_mul;
using lvi_marg_math::mat3_mul;
using lvi_marg_math::mat3_tmul;
using lvi_marg_math::mat3_tvec;
using lvi_marg_math::mat3_vec;
namespace pm = lvi_preint_math;

constexpr int BAND = 5, BW = BAND + 1;
constexpr int NB_LINEAR = 4, NB_REFINE = 3, PASSES = 4, SYSTEMS = 1 + PASSES;
constexpr int OK = 0, GRAVITY_NORM = 1, NEGATIVE_SCALE = 2, NEGATIVE_SCALE_REFINED = 3, SINGULAR = 4, TOO_FEW = 5;
constexpr int APPLY_OPPOSITE = 1;

// what the alignment reads of a frame's preintegration
struct Pre {
    double sum_dt, delta_p[3], delta_q[4], delta_v[3];
};

LVI_MARG_HD bool positive_finite(double v) { return v > 0. && v <= DBL_MAX; }
LVI_MARG_HD bool all_finite(const double* v, int n)
{
    for (int k = 0; k < n; k++)
        if (!(std::fabs(v[k]) <= DBL_MAX)) return false;
    return true;
}

// Eigen's Quaternion(Matrix3): the trace branch and the three others
LVI_MARG_HD void rot_to_quat(const double* R, double* q)
{
    double t = R[0] + R[4] + R[8];
    if (t > 0.) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[3 * k + j] - R[3 * j + k]) * t;
        q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
        q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
    }
}

LVI_MARG_HD double norm3(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
// Eigen's normalized(): the vector itself when its squared norm is not > 0
LVI_MARG_HD void normalized3(const double* v, double* o)
{
    const double n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    if (n2 > 0.) { const double n = std::sqrt(n2); o[0] = v[0] / n; o[1] = v[1] / n; o[2] = v[2] / n; }
    else { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; }
}

// ---- solveGyroscopeBias (:3-36) -------------------------------------------------------------------------------------
// one pair: out[0..8] = tmp_A' tmp_A, out[9..11] = tmp_A' tmp_b with tmp_A = jacobian(O_R, O_BG) of frame j
LVI_MARG_HD void gyro_pair(const double* Ri, const double* Rj, const double* delta_q, const double* jacobian, double* out)
{
    double Rij[9], qij[4], qi[4], e[4], tb[3];
    mat3_tmul(Ri, Rj, Rij);
    rot_to_quat(Rij, qij);
    quat_inv(delta_q, qi);
    quat_mul(qi, qij, e);
    for (int k = 0; k < 3; k++) tb[k] = 2. * e[k];
    const double* A = jacobian + pm::N * lvi_imu_math::O_R + lvi_imu_math::O_BG;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) out[3 * r + c] = A[r] * A[c] + A[pm::N + r] * A[pm::N + c] + A[2 * pm::N + r] * A[2 * pm::N + c];
        out[9 + r] = A[r] * tb[0] + A[pm::N + r] * tb[1] + A[2 * pm::N + r] * tb[2];
    }
}

// ---- the symmetric solve: dense statement ---------------------------------------------------------------------------
// unpivoted L D L' of the n x n matrix A (row-major, lower triangle read, overwritten by L and d) and the solve of b into x;
// false, and x untouched, on a pivot that is not finite or not > 0; *min_pivot: the smallest pivot met
LVI_MARG_HD bool ldl_dense(int n, double* A, const double* b, double* x, double* min_pivot)
{
    double mp = DBL_MAX;
    for (int j = 0; j < n; j++) {
        double v = A[n * j + j];
        for (int k = 0; k < j; k++) { const double l = A[n * j + k]; v = v - (l * A[n * k + k]) * l; }
        if (!positive_finite(v)) { *min_pivot = 0.; return false; }
        if (v < mp) mp = v;
        for (int i = j + 1; i < n; i++) {
            double s = A[n * i + j];
            for (int k = 0; k < j; k++) s = s - (A[n * i + k] * A[n * k + k]) * A[n * j + k];
            A[n * i + j] = s / v;
        }
        A[n * j + j] = v;
    }
    *min_pivot = mp;
    for (int i = 0; i < n; i++) {
        double z = b[i];
        for (int k = 0; k < i; k++) z = z - A[n * i + k] * x[k];
        x[i] = z;
    }
    for (int i = 0; i < n; i++) x[i] = x[i] / A[n * i + i];
    for (int i = n - 1; i >= 0; i--) {
        double z = x[i];
        for (int k = i + 1; k < n; k++) z = z - A[n * k + i] * x[k];
        x[i] = z;
    }
    return true;
}

// the 3 x 3 solve of solveGyroscopeBias: delta_bg is zero, and the reason SINGULAR, on a bad pivot or a solution that is not finite
LVI_MARG_HD int gyro_solve(double* A, const double* b, double* delta_bg, double* min_pivot)
{
    double x[3] = {0., 0., 0.};
    const bool ok = ldl_dense(3, A, b, x, min_pivot) && all_finite(x, 3);
    for (int k = 0; k < 3; k++) delta_bg[k] = ok ? x[k] : 0.;
    return ok ? OK : SINGULAR;
}

// ---- the compact system ---------------------------------------------------------------------------------------------
LVI_MARG_HD int sys_doubles(int nd, int nb) { return BW * nd + (nb + 2) * (nd + nb); }     // band | bord | b | x
LVI_MARG_HD int off_bord(int nd) { return BW * nd; }
LVI_MARG_HD int off_b(int nd, int nb) { return BW * nd + nb * (nd + nb); }
LVI_MARG_HD int off_x(int nd, int nb) { return BW * nd + (nb + 1) * (nd + nb); }

// d[k] of a compact system during and after the factorisation
LVI_MARG_HD double c_d(const double* band, const double* bord, int nd, int n, int k) { return k < nd ? band[BW * k] : bord[n * (k - nd) + k]; }

// The rows and columns inside the band, with the indices written out: the same terms in the same order as the general
// forms below, which they serve.  k ascending is d = j - k descending.
LVI_MARG_HD double band_pivot(const double* band, int j)
{
    double v = band[BW * j];
    for (int d = j < BAND ? j : BAND; d >= 1; d--) { const double l = band[BW * j + d]; v = v - (l * band[BW * (j - d)]) * l; }
    return v;
}
LVI_MARG_HD double band_entry(const double* band, int i, int j, double v)          // j < i < nd, i - j <= BAND
{
    double s = band[BW * i + (i - j)];
    for (int k = i > BAND ? i - BAND : 0; k < j; k++) s = s - (band[BW * i + (i - k)] * band[BW * k]) * band[BW * j + (j - k)];
    return s / v;
}
LVI_MARG_HD double bord_entry(const double* band, const double* row, int j, double v)   // row = bord + n kb, j < nd
{
    double s = row[j];
    for (int k = j > BAND ? j - BAND : 0; k < j; k++) s = s - (row[k] * band[BW * k]) * band[BW * j + (j - k)];
    return s / v;
}
// the pivot of column j: every L[j][k] is final
LVI_MARG_HD double c_pivot(const double* band, const double* bord, int nd, int n, int j)
{
    if (j < nd) return band_pivot(band, j);
    const double* row = bord + n * (j - nd);
    double v = row[j];
    for (int k = 0; k < nd; k++) { const double l = row[k]; v = v - (l * band[BW * k]) * l; }
    for (int k = nd; k < j; k++) { const double l = row[k]; v = v - (l * bord[n * (k - nd) + k]) * l; }
    return v;
}
// L[i][j] for a row i > j inside the pattern, v the pivot of column j
LVI_MARG_HD double c_entry(const double* band, const double* bord, int nd, int n, int i, int j, double v)
{
    if (i < nd) return band_entry(band, i, j, v);
    const double* row = bord + n * (i - nd);
    if (j < nd) return bord_entry(band, row, j, v);
    const double* rj = bord + n * (j - nd);
    double s = row[j];
    for (int k = 0; k < nd; k++) s = s - (row[k] * band[BW * k]) * rj[k];
    for (int k = nd; k < j; k++) s = s - (row[k] * bord[n * (k - nd) + k]) * rj[k];
    return s / v;
}
LVI_MARG_HD void c_store(double* band, double* bord, int nd, int n, int i, int j, double v)
{
    if (i < nd) band[BW * i + (i - j)] = v; else bord[n * (i - nd) + j] = v;
}
// the rows below j that hold an entry in column j: `slot` 0..BAND + nb - 1 -> the row, or -1
LVI_MARG_HD int c_row(int nd, int nb, int j, int slot)
{
    if (slot < BAND) { const int i = j + 1 + slot; return (j < nd && i < nd) ? i : -1; }
    const int i = nd + (slot - BAND);
    return (slot - BAND < nb && i > j) ? i : -1;
}
// forward, diagonal and backward substitution on the factored system, each in place on x, which holds b on entry; the
// diagonal step is one division per entry and may run on any number of threads
LVI_MARG_HD void c_forward(const double* band, const double* bord, int nd, int nb, double* x)
{
    const int n = nd + nb;
    for (int i = 0; i < nd; i++) {
        double z = x[i];
        for (int k = i > BAND ? i - BAND : 0; k < i; k++) z = z - band[BW * i + (i - k)] * x[k];
        x[i] = z;
    }
    for (int i = nd; i < n; i++) {
        const double* row = bord + n * (i - nd);
        double z = x[i];
        for (int k = 0; k < i; k++) z = z - row[k] * x[k];
        x[i] = z;
    }
}
LVI_MARG_HD void c_diag(const double* band, const double* bord, int nd, int n, int i, double* x) { x[i] = x[i] / c_d(band, bord, nd, n, i); }
LVI_MARG_HD void c_backward(const double* band, const double* bord, int nd, int nb, double* x)
{
    const int n = nd + nb;
    for (int i = n - 1; i >= nd; i--) {
        double z = x[i];
        for (int k = i + 1; k < n; k++) z = z - bord[n * (k - nd) + i] * x[k];
        x[i] = z;
    }
    for (int i = nd - 1; i >= 0; i--) {
        double z = x[i];
        for (int k = i + 1; k <= i + BAND && k < nd; k++) z = z - band[BW * k + (k - i)] * x[k];
        for (int kb = 0; kb < nb; kb++) z = z - bord[n * kb + i] * x[nd + kb];
        x[i] = z;
    }
}
LVI_MARG_HD void c_solve(const double* band, const double* bord, int nd, int nb, double* x)
{
    const int n = nd + nb;
    c_forward(band, bord, nd, nb, x);
    for (int i = 0; i < n; i++) c_diag(band, bord, nd, n, i, x);
    c_backward(band, bord, nd, nb, x);
}
// the whole on one thread; band and bord are overwritten, x receives the solution
LVI_MARG_HD bool ldl_band(int nd, int nb, double* band, double* bord, const double* b, double* x, double* min_pivot)
{
    const int n = nd + nb;
    double mp = DBL_MAX;
    *min_pivot = 0.;
    if (2 * (nd - 3) < n) return false;                              // 6 (F - 1) equations for n unknowns
    for (int j = 0; j < n; j++) {
        const double v = c_pivot(band, bord, nd, n, j);
        if (!positive_finite(v)) return false;
        if (v < mp) mp = v;
        for (int s = 0; s < BAND + nb; s++) { const int i = c_row(nd, nb, j, s); if (i >= 0) c_store(band, bord, nd, n, i, j, c_entry(band, bord, nd, n, i, j, v)); }
        c_store(band, bord, nd, n, j, j, v);
    }
    *min_pivot = mp;
    for (int i = 0; i < n; i++) x[i] = b[i];
    c_solve(band, bord, nd, nb, x);
    return all_finite(x, n);                                         // a right-hand side that is not finite
}
// compact -> dense (row-major n x n, both triangles)
LVI_MARG_HD void c_expand(int nd, int nb, const double* band, const double* bord, double* A)
{
    const int n = nd + nb;
    for (int k = 0; k < n * n; k++) A[k] = 0.;
    for (int i = 0; i < nd; i++)
        for (int d = 0; d <= BAND && d <= i; d++) A[n * i + i - d] = A[n * (i - d) + i] = band[BW * i + d];
    for (int k = 0; k < nb; k++)
        for (int j = 0; j <= nd + k; j++) A[n * (nd + k) + j] = A[n * j + nd + k] = bord[n * k + j];
}

// ---- TangentBasis (:39-52) ------------------------------------------------------------------------------------------
// lxly row-major 3 x 2
LVI_MARG_HD void tangent_basis(const double* g0, double* lxly)
{
    double a[3], t[3] = {0., 0., 1.}, u[3], b[3];
    normalized3(g0, a);
    if (a[0] == t[0] && a[1] == t[1] && a[2] == t[2]) { t[0] = 1.; t[2] = 0.; }
    const double d = a[0] * t[0] + a[1] * t[1] + a[2] * t[2];
    for (int k = 0; k < 3; k++) u[k] = t[k] - a[k] * d;
    normalized3(u, b);
    const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    for (int k = 0; k < 3; k++) { lxly[2 * k] = b[k]; lxly[2 * k + 1] = c[k]; }
}

// ---- one pair of LinearAlignment (:141-165, lxly == nullptr) or of RefineGravity (:78-103) ---------------------------
// rA (6 + nb) x (6 + nb) row-major, rb [6 + nb]; nb = 4 without lxly, 3 with
LVI_MARG_HD void pair_system(const double* Ri, const double* Ti, const double* Rj, const double* Tj, const Pre& pj, const double* TIC, const double* lxly,
                             const double* g0, double* rA, double* rb)
{
    const int nb = lxly ? NB_REFINE : NB_LINEAR, W = 6 + nb;
    const double dt = pj.sum_dt;
    double tA[6 * 10], tb[6], Rij[9], M[9], Md[9], d[3], u[3], v[3];
    for (int k = 0; k < 6 * W; k++) tA[k] = 0.;
    mat3_tmul(Ri, Rj, Rij);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { M[3 * r + c] = Ri[3 * c + r] * dt * dt / 2; Md[3 * r + c] = Ri[3 * c + r] * dt; }
    for (int k = 0; k < 3; k++) d[k] = Tj[k] - Ti[k];
    mat3_tvec(Ri, d, u);
    mat3_vec(Rij, TIC, v);
    for (int r = 0; r < 3; r++) {
        tA[W * r + r] = -dt;
        tA[W * (3 + r) + r] = -1.;
        for (int c = 0; c < 3; c++) tA[W * (3 + r) + 3 + c] = Rij[3 * r + c];
        tA[W * r + W - 1] = u[r] / 100.0;
        tb[r] = pj.delta_p[r] + v[r] - TIC[r];
        tb[3 + r] = pj.delta_v[r];
        if (!lxly) {
            for (int c = 0; c < 3; c++) { tA[W * r + 6 + c] = M[3 * r + c]; tA[W * (3 + r) + 6 + c] = Md[3 * r + c]; }
        } else {
            for (int c = 0; c < 2; c++) {
                tA[W * r + 6 + c] = M[3 * r] * lxly[c] + M[3 * r + 1] * lxly[2 + c] + M[3 * r + 2] * lxly[4 + c];
                tA[W * (3 + r) + 6 + c] = Md[3 * r] * lxly[c] + Md[3 * r + 1] * lxly[2 + c] + Md[3 * r + 2] * lxly[4 + c];
            }
            tb[r] = tb[r] - (M[3 * r] * g0[0] + M[3 * r + 1] * g0[1] + M[3 * r + 2] * g0[2]);
            tb[3 + r] = tb[3 + r] - (Md[3 * r] * g0[0] + Md[3 * r + 1] * g0[1] + Md[3 * r + 2] * g0[2]);
        }
    }
    for (int a = 0; a < W; a++) {
        for (int c = 0; c < W; c++) {
            double s = 0.;
            for (int k = 0; k < 6; k++) s = s + tA[W * k + a] * tA[W * k + c];
            rA[W * a + c] = s;
        }
        double s = 0.;
        for (int k = 0; k < 6; k++) s = s + tA[W * k + a] * tb[k];
        rb[a] = s;
    }
}

// adds pair p onto the compact system (ascending p is the caller's order)
LVI_MARG_HD void scatter_pair(int p, int nd, int nb, const double* rA, const double* rb, double* band, double* bord, double* b)
{
    const int W = 6 + nb, n = nd + nb;
    for (int a = 0; a < 6; a++) {
        for (int c = 0; c <= a; c++) band[BW * (3 * p + a) + (a - c)] = band[BW * (3 * p + a) + (a - c)] + rA[W * a + c];
        b[3 * p + a] = b[3 * p + a] + rb[a];
    }
    for (int k = 0; k < nb; k++) {
        for (int c = 0; c < 6; c++) bord[n * k + 3 * p + c] = bord[n * k + 3 * p + c] + rA[W * (6 + k) + c];
        for (int c = 0; c <= k; c++) bord[n * k + nd + c] = bord[n * k + nd + c] + rA[W * (6 + k) + 6 + c];
        b[nd + k] = b[nd + k] + rb[6 + k];
    }
}

// ---- what follows a solve -------------------------------------------------------------------------------------------
// LinearAlignment's gates (:179-188): g = x.segment<3>(n - 4), s = x(n - 1) / 100 -> the reason; g0 = g.normalized() * |G|
LVI_MARG_HD int linear_gate(const double* x, int n, const double* G, double* g, double* s, double* g0)
{
    for (int k = 0; k < 3; k++) g[k] = x[n - 4 + k];
    *s = x[n - 1] / 100.0;
    const double gn = norm3(G);
    double a[3];
    normalized3(g, a);
    for (int k = 0; k < 3; k++) g0[k] = a[k] * gn;
    if (std::fabs(norm3(g) - gn) > 1.0) return GRAVITY_NORM;
    if (*s < 0) return NEGATIVE_SCALE;
    return OK;
}
// :117-118: g0 = (g0 + lxly dg).normalized() * |G|
LVI_MARG_HD void refine_step(const double* x, int n, const double* lxly, const double* G, double* g0)
{
    const double dg0 = x[n - 3], dg1 = x[n - 2], gn = norm3(G);
    double t[3], a[3];
    for (int k = 0; k < 3; k++) t[k] = g0[k] + (lxly[2 * k] * dg0 + lxly[2 * k + 1] * dg1);
    normalized3(t, a);
    for (int k = 0; k < 3; k++) g0[k] = a[k] * gn;
}

// ---- the excitation check (estimator.cpp:273-300); sum_g starts at 0; pre [m]: the frames after the first -------------
LVI_MARG_HD double excitation(const Pre* pre, int m)
{
    double sum[3] = {0., 0., 0.}, aver[3], var = 0.;
    for (int i = 0; i < m; i++)
        for (int k = 0; k < 3; k++) sum[k] = sum[k] + pre[i].delta_v[k] / pre[i].sum_dt;
    for (int k = 0; k < 3; k++) aver[k] = sum[k] * 1.0 / m;
    for (int i = 0; i < m; i++) {
        double d[3];
        for (int k = 0; k < 3; k++) d[k] = pre[i].delta_v[k] / pre[i].sum_dt - aver[k];
        var = var + (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    }
    return std::sqrt(var / m);
}

// ---- the tail of visualInitialAlign (estimator.cpp:450-486), host only in the library: atan2, sin, cos ----------------
// yaw of Utility::R2ypr in degrees
LVI_MARG_HD double yaw_deg(const double* R) { return std::atan2(R[3], R[0]) / M_PI * 180.0; }
// Utility::ypr2R({yaw_deg, 0, 0}) * R
LVI_MARG_HD void yaw_left(double deg, const double* R, double* o)
{
    const double y = deg / 180.0 * M_PI, c = std::cos(y), s = std::sin(y);
    const double Rz[9] = {c, -s, 0., s, c, 0., 0., 0., 1.};
    mat3_mul(Rz, R, o);
}
// Utility::g2R (utility.cpp:3-13).  Quaterniond::FromTwoVectors picks, for nearly opposite vectors (their dot product below
// -1 + 1e-12), an axis from an SVD; here the rotation by pi about x is taken instead (q = 1 0 0 0) and *flags gets
// APPLY_OPPOSITE: a stated choice for a gravity that points along -z of the camera frame.
LVI_MARG_HD void g2R(const double* g, double* R0, int* flags)
{
    double a[3], q[4], Rq[9];
    normalized3(g, a);
    const double c = a[2];                                            // ng2 = 0 0 1
    if (c < -1.0 + 1e-12) { q[0] = 1.; q[1] = q[2] = q[3] = 0.; *flags |= APPLY_OPPOSITE; }
    else {
        const double s = std::sqrt((1.0 + c) * 2.0), inv = 1.0 / s;
        q[0] = a[1] * inv; q[1] = -a[0] * inv; q[2] = 0. * inv; q[3] = s * 0.5;    // a x (0 0 1) = (a1, -a0, 0)
    }
    lvi_marg_math::quat_to_rot(q, Rq);
    yaw_left(-yaw_deg(Rq), Rq, R0);
}
// Ps [fc + 1][3], Rs [fc + 1][9], Vs [fc + 1][3] (written for the key frames met, at most fc + 1), x with s at x[n_x - 1],
// g [3] in and out; key_R [n_key][9]: R of the list's key frames in list order (the kv walk of :457-466)
LVI_MARG_HD void apply(int frame_count, const double* TIC, double* Ps, double* Rs, double* Vs, const double* x, int n_x, double* g, const double* key_R, int n_key,
                       double* rot_diff, int* flags)
{
    const double s = x[n_x - 1];
    double r0[3], p0[3];
    mat3_vec(Rs, TIC, r0);
    for (int k = 0; k < 3; k++) p0[k] = s * Ps[k] - r0[k];
    for (int i = frame_count; i >= 0; i--) {
        double ri[3];
        mat3_vec(Rs + 9 * i, TIC, ri);
        for (int k = 0; k < 3; k++) Ps[3 * i + k] = s * Ps[3 * i + k] - ri[k] - p0[k];
    }
    for (int kv = 0; kv < n_key && kv <= frame_count; kv++) mat3_vec(key_R + 9 * kv, x + 3 * kv, Vs + 3 * kv);
    double R0[9], RR[9], t[9];
    *flags = 0;
    g2R(g, R0, flags);
    mat3_mul(R0, Rs, RR);
    yaw_left(-yaw_deg(RR), R0, rot_diff);
    double gn[3];
    mat3_vec(rot_diff, g, gn);
    for (int k = 0; k < 3; k++) g[k] = gn[k];
    for (int i = 0; i <= frame_count; i++) {
        double v[3];
        mat3_vec(rot_diff, Ps + 3 * i, v);
        for (int k = 0; k < 3; k++) Ps[3 * i + k] = v[k];
        mat3_mul(rot_diff, Rs + 9 * i, t);
        for (int k = 0; k < 9; k++) Rs[9 * i + k] = t[k];
        mat3_vec(rot_diff, Vs + 3 * i, v);
        for (int k = 0; k < 3; k++) Vs[3 * i + k] = v[k];
    }
}

// ---- the repropagation of one frame on the host: IntegrationBase::repropagate without the covariance ------------------
// work: pm::WORK_DOUBLES (F, V and the new jacobian; T is not used)
LVI_MARG_HD void repropagate(pm::State& s, double* jacobian, const double* lin_acc, const double* lin_gyr, const double* ba, const double* bg, int n,
                             const double* smp7, double* work)
{
    pm::state_reset(s, lin_acc, lin_gyr, ba, bg);
    for (int k = 0; k < pm::N * pm::N; k++) jacobian[k] = (k / pm::N == k % pm::N) ? 1. : 0.;
    double *Fm = work, *Vm = work + 225, *Jn = work + 720;
    pm::StepGeom g;
    for (int t = 0; t < n; t++) {
        const double* x = smp7 + 7 * t;
        pm::step_state(s, x[0], x + 1, x + 4, g);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) pm::build_entry(g, i, j, Fm, Vm);
        for (int r = 0; r < pm::N; r++)
            for (int c = 0; c < pm::N; c++) Jn[pm::N * r + c] = pm::f_dot(Fm, r, jacobian, c);
        for (int k = 0; k < pm::N * pm::N; k++) jacobian[k] = Jn[k];
    }
}

// ---- VisualIMUAlignment on one thread: the statement the device is held to, and the host column of tools/diag ---------
struct Frame {
    double R[9], T[3];
    Pre pre;                          // of frame j >= 1
    const double* jacobian;           // 225, after the repropagation
};
struct Result {
    int ok, reason, n_state, built;   // built: the systems built and factored, 0..SYSTEMS
    double delta_bg[3], s, g_linear[3], g[3], min_pivot[1 + SYSTEMS];
};
// the gyro stage over frames whose jacobians are the present ones -> delta_bg (zero, and SINGULAR, on a bad pivot)
LVI_MARG_HD int gyro_bias(const Frame* f, int F, double* delta_bg, double* min_pivot)
{
    double A[9] = {0.}, b[3] = {0.}, o[12];
    for (int p = 0; p + 1 < F; p++) {
        gyro_pair(f[p].R, f[p + 1].R, f[p + 1].pre.delta_q, f[p + 1].jacobian, o);
        for (int k = 0; k < 9; k++) A[k] = A[k] + o[k];
        for (int k = 0; k < 3; k++) b[k] = b[k] + o[9 + k];
    }
    return gyro_solve(A, b, delta_bg, min_pivot);
}
// LinearAlignment with RefineGravity over the repropagated frames.  sys: SYSTEMS compact systems of sys_doubles(3 F, 4)
// doubles each (every one kept as built: band | bord | b | x); work: BW nd + 4 n doubles for the factor.
LVI_MARG_HD void linear_alignment(const Frame* f, int F, const double* TIC, const double* G, double* sys, double* work, Result& r)
{
    const int nd = 3 * F, stride = sys_doubles(nd, NB_LINEAR);
    double g0[3] = {0., 0., 0.}, lxly[6], rA[100], rb[10];
    r.reason = OK; r.n_state = nd + NB_LINEAR; r.s = 0.; r.built = 0;
    for (int k = 0; k < 3; k++) r.g_linear[k] = r.g[k] = 0.;
    for (int k = 0; k < SYSTEMS; k++) r.min_pivot[1 + k] = 0.;
    for (int w = 0; w < SYSTEMS; w++) {
        const int nb = w == 0 ? NB_LINEAR : NB_REFINE, n = nd + nb;
        double *S = sys + (size_t)stride * w, *band = S, *bord = S + off_bord(nd), *b = S + off_b(nd, nb), *x = S + off_x(nd, nb);
        const double* prev = w >= 2 ? S - stride : nullptr;
        for (int k = 0; k < off_x(nd, nb); k++) S[k] = prev ? prev[k] : 0.;
        for (int k = 0; k < n; k++) x[k] = 0.;
        if (w >= 1) tangent_basis(g0, lxly);
        for (int p = 0; p + 1 < F; p++) {
            pair_system(f[p].R, f[p].T, f[p + 1].R, f[p + 1].T, f[p + 1].pre, TIC, w >= 1 ? lxly : nullptr, g0, rA, rb);
            scatter_pair(p, nd, nb, rA, rb, band, bord, b);
        }
        for (int k = 0; k < off_x(nd, nb); k++) S[k] = S[k] * 1000.0;
        double *fb = work, *fo = work + BW * nd;
        for (int k = 0; k < BW * nd; k++) fb[k] = band[k];
        for (int k = 0; k < nb * n; k++) fo[k] = bord[k];
        r.built = w + 1;
        if (!ldl_band(nd, nb, fb, fo, b, x, &r.min_pivot[1 + w])) {
            r.reason = SINGULAR; r.n_state = nd + NB_LINEAR; r.s = 0.; r.min_pivot[1 + w] = 0.;
            for (int k = 0; k < 3; k++) r.g_linear[k] = r.g[k] = 0.;
            for (int k = 0; k < n; k++) x[k] = 0.;
            return;
        }
        if (w == 0) {
            r.n_state = n;
            r.reason = linear_gate(x, n, G, r.g_linear, &r.s, g0);
            for (int k = 0; k < 3; k++) r.g[k] = r.g_linear[k];
            if (r.reason != OK) return;
        } else {
            refine_step(x, n, lxly, G, g0);
        }
    }
    const int n = nd + NB_REFINE;
    double* x = sys + (size_t)stride * (SYSTEMS - 1) + off_x(nd, NB_REFINE);
    x[n - 1] = x[n - 1] / 100.0;
    r.n_state = n; r.s = x[n - 1];
    for (int k = 0; k < 3; k++) r.g[k] = g0[k];
    if (r.s < 0.0) r.reason = NEGATIVE_SCALE_REFINED;
}

}  // namespace lvi_align_math
