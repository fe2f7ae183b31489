// The arithmetic of lvi_pnp.hip (include/lvi_pnp.h): epnp::compute_pose of OpenCV 4.5.x calib3d/src/epnp.cpp
// with fu = fv = 1, uc = vc = 0, restated with decompositions of a fixed operation order, and the reprojection error of
// PnPRansacCallback::computeError.  Everything is double; only + - * / and sqrt are used, one rounding each (the library
// is built with -ffp-contract=off), so tests/pnp_ref.py, which performs the same operations in the same order, produces
// the same bits.  The functions compile for the host as well: tests run them under the host sanitizers.
//
// Decompositions (the restatement's own; OpenCV's Jacobi SVD and Householder solve are not reproduced):
//   pnp_eig3     symmetric 3x3, cyclic Jacobi, PNP_SWEEPS3 sweeps, rows then columns
//   jacobi12_*   symmetric 12x12, round-robin Jacobi: 11 rounds of 6 disjoint pairs per sweep, all six (c, s) from the
//                current matrix, then the row rotations, then the column rotations; one entry per call, so that a wave
//                spreads the entries over its lanes and a host loop visits them one by one
//   pnp_inv3     Gauss-Jordan with partial pivoting; an exactly zero pivot = no model
//   pnp_lstsq    Householder QR, column by column, no pivoting
//   pnp_polar3   R = U V' of a 3x3 SVD by one-sided Jacobi, PNP_SWEEPS3 sweeps
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define LVI_PNP_HD __host__ __device__ inline
#else
#define LVI_PNP_HD inline
#endif

namespace lvi_pnp_math {

constexpr int PNP_SWEEPS12 = 8;
constexpr int PNP_SWEEPS3 = 8;
constexpr int PNP_GN_STEPS = 5;

// the Jacobi rotation that zeroes a_pq
LVI_PNP_HD void pnp_rot(double apq, double app, double aqq, double* c, double* s)
{
    if (apq == 0.) { *c = 1.; *s = 0.; return; }
    const double theta = (aqq - app) / (2. * apq);
    const double t = (theta < 0 ? -1. : 1.) / (fabs(theta) + sqrt(theta * theta + 1.));
    *c = 1. / sqrt(t * t + 1.);
    *s = t * *c;
}

// symmetric S [3][3] (destroyed) -> lam [3] descending (ties to the lower index), E [3][3] with the eigenvectors in columns
LVI_PNP_HD void pnp_eig3(double* a, double* lam, double* E)
{
    double v[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
    for (int sw = 0; sw < PNP_SWEEPS3; sw++)
        for (int pr = 0; pr < 3; pr++) {
            const int p = pr == 2 ? 1 : 0, q = pr == 0 ? 1 : 2;
            double c, s;
            pnp_rot(a[3 * p + q], a[3 * p + p], a[3 * q + q], &c, &s);
            for (int j = 0; j < 3; j++) { const double x = a[3 * p + j], y = a[3 * q + j]; a[3 * p + j] = c * x - s * y; a[3 * q + j] = s * x + c * y; }
            for (int i = 0; i < 3; i++) { const double x = a[3 * i + p], y = a[3 * i + q]; a[3 * i + p] = c * x - s * y; a[3 * i + q] = s * x + c * y; }
            for (int i = 0; i < 3; i++) { const double x = v[3 * i + p], y = v[3 * i + q]; v[3 * i + p] = c * x - s * y; v[3 * i + q] = s * x + c * y; }
        }
    const double d[3] = {a[0], a[4], a[8]};
    bool used[3] = {false, false, false};
    for (int k = 0; k < 3; k++) {
        int best = -1;
        for (int i = 0; i < 3; i++) {
            if (used[i]) continue;
            if (best < 0 || d[i] > d[best]) best = i;
        }
        used[best] = true;
        lam[k] = d[best];
        for (int r = 0; r < 3; r++) E[3 * r + k] = v[3 * r + best];
    }
}

// ---- the 12x12 round-robin Jacobi, one entry at a time --------------------------------------------------------------
// pair k (0..5) of round r (0..10): (r, 11), then ((r + k) % 11, (r - k + 11) % 11) with p < q
LVI_PNP_HD void jacobi12_pair(int r, int k, int* p, int* q)
{
    if (k == 0) { *p = r; *q = 11; return; }
    const int a = (r + k) % 11, b = (r - k + 11) % 11;
    *p = a < b ? a : b; *q = a < b ? b : a;
}
// the pair of index i in round r, and i's partner
LVI_PNP_HD void jacobi12_partner(int r, int i, int* k, int* partner)
{
    if (i == 11) { *k = 0; *partner = r; return; }
    if (i == r) { *k = 0; *partner = 11; return; }
    const int d = (i - r + 11) % 11;
    if (d <= 5) { *k = d; *partner = (r - d + 11) % 11; }
    else { *k = 11 - d; *partner = (r + 11 - d) % 11; }
}
// entry (i, j) of J'A: rows p and q of every pair mix; cs [6][2] = (c, s) per pair
LVI_PNP_HD double jacobi12_row(const double* A, int ld, const double* cs, int r, int i, int j)
{
    int k, o;
    jacobi12_partner(r, i, &k, &o);
    const double c = cs[2 * k], s = cs[2 * k + 1];
    return i < o ? c * A[ld * i + j] - s * A[ld * o + j] : s * A[ld * o + j] + c * A[ld * i + j];
}
// entry (i, j) of A J
LVI_PNP_HD double jacobi12_col(const double* A, int ld, const double* cs, int r, int i, int j)
{
    int k, o;
    jacobi12_partner(r, j, &k, &o);
    const double c = cs[2 * k], s = cs[2 * k + 1];
    return j < o ? c * A[ld * i + j] - s * A[ld * i + o] : s * A[ld * i + o] + c * A[ld * i + j];
}

// indices of v[0..3]: the four smallest eigenvalues, v[0] the smallest; among equals the higher index first (the tail of a
// descending sort whose ties go to the lower index)
LVI_PNP_HD void pnp_smallest4(const double* lam, int* idx)
{
    bool used[12];
    for (int i = 0; i < 12; i++) used[i] = false;
    for (int k = 0; k < 4; k++) {
        int best = -1;
        for (int i = 0; i < 12; i++) {
            if (used[i]) continue;
            if (best < 0 || lam[i] <= lam[best]) best = i;
        }
        used[best] = true;
        idx[k] = best;
    }
}

// ci = inverse of m (both [3][3]); false on an exactly zero pivot
LVI_PNP_HD bool pnp_inv3(const double* m, double* ci)
{
    double a[18];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { a[6 * i + j] = m[3 * i + j]; a[6 * i + 3 + j] = i == j ? 1. : 0.; }
    for (int c = 0; c < 3; c++) {
        int p = c;
        double best = fabs(a[6 * c + c]);
        for (int i = c + 1; i < 3; i++) if (fabs(a[6 * i + c]) > best) { best = fabs(a[6 * i + c]); p = i; }
        if (best == 0) return false;
        if (p != c) for (int j = 0; j < 6; j++) { const double t = a[6 * c + j]; a[6 * c + j] = a[6 * p + j]; a[6 * p + j] = t; }
        const double d = a[6 * c + c];
        for (int j = 0; j < 6; j++) a[6 * c + j] = a[6 * c + j] / d;
        for (int i = 0; i < 3; i++) {
            if (i == c) continue;
            const double f = a[6 * i + c];
            for (int j = 0; j < 6; j++) a[6 * i + j] = a[6 * i + j] - f * a[6 * c + j];
        }
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) ci[3 * i + j] = a[6 * i + 3 + j];
    return true;
}

// min |A x - b|, A [6][NC] and b [6] destroyed.  A column that is exactly zero from the diagonal down: x = 0.
template <int NC>
LVI_PNP_HD void pnp_lstsq(double* a, double* b, double* x)
{
    constexpr int NR = 6;
    double a1[NC], a2[NC];
    for (int k = 0; k < NC; k++) {
        double eta = 0.;
        for (int i = k; i < NR; i++) { const double e = fabs(a[NC * i + k]); if (eta < e) eta = e; }
        if (eta == 0) { for (int i = 0; i < NC; i++) x[i] = 0.; return; }
        const double inv_eta = 1. / eta;
        double sum2 = 0.;
        for (int i = k; i < NR; i++) { a[NC * i + k] = a[NC * i + k] * inv_eta; sum2 = sum2 + a[NC * i + k] * a[NC * i + k]; }
        double sigma = sqrt(sum2);
        if (a[NC * k + k] < 0) sigma = -sigma;
        a[NC * k + k] = a[NC * k + k] + sigma;
        a1[k] = sigma * a[NC * k + k];
        a2[k] = -eta * sigma;
        for (int j = k + 1; j < NC; j++) {
            double s = 0.;
            for (int i = k; i < NR; i++) s = s + a[NC * i + k] * a[NC * i + j];
            const double tau = s / a1[k];
            for (int i = k; i < NR; i++) a[NC * i + j] = a[NC * i + j] - tau * a[NC * i + k];
        }
    }
    for (int j = 0; j < NC; j++) {
        double tau = 0.;
        for (int i = j; i < NR; i++) tau = tau + a[NC * i + j] * b[i];
        tau = tau / a1[j];
        for (int i = j; i < NR; i++) b[i] = b[i] - tau * a[NC * i + j];
    }
    for (int i = NC - 1; i >= 0; i--) {
        double s = 0.;
        for (int j = i + 1; j < NC; j++) s = s + a[NC * i + j] * x[j];
        x[i] = (b[i] - s) / a2[i];
    }
}

// R = U V' of the SVD of b [3][3] (destroyed)
LVI_PNP_HD void pnp_polar3(double* b, double* R)
{
    double v[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
    for (int sw = 0; sw < PNP_SWEEPS3; sw++)
        for (int pr = 0; pr < 3; pr++) {
            const int p = pr == 2 ? 1 : 0, q = pr == 0 ? 1 : 2;
            const double al = b[p] * b[p] + b[3 + p] * b[3 + p] + b[6 + p] * b[6 + p];
            const double be = b[q] * b[q] + b[3 + q] * b[3 + q] + b[6 + q] * b[6 + q];
            const double ga = b[p] * b[q] + b[3 + p] * b[3 + q] + b[6 + p] * b[6 + q];
            double c, s;
            pnp_rot(ga, al, be, &c, &s);
            for (int i = 0; i < 3; i++) { const double x = b[3 * i + p], y = b[3 * i + q]; b[3 * i + p] = c * x - s * y; b[3 * i + q] = s * x + c * y; }
            for (int i = 0; i < 3; i++) { const double x = v[3 * i + p], y = v[3 * i + q]; v[3 * i + p] = c * x - s * y; v[3 * i + q] = s * x + c * y; }
        }
    for (int j = 0; j < 3; j++) {
        const double nrm = sqrt(b[j] * b[j] + b[3 + j] * b[3 + j] + b[6 + j] * b[6 + j]);
        for (int i = 0; i < 3; i++) b[3 * i + j] = b[3 * i + j] / nrm;
    }
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) R[3 * i + k] = b[3 * i] * v[3 * k] + b[3 * i + 1] * v[3 * k + 1] + b[3 * i + 2] * v[3 * k + 2];
}

// ---- epnp ------------------------------------------------------------------------------------------------------------
// choose_control_points + compute_barycentric_coordinates: pw [n][3] -> cws [4][3], alphas [n][4]; false = no model
LVI_PNP_HD bool pnp_control_points(const double* pw, int n, double* cws, double* alphas)
{
    double c0[3] = {0., 0., 0.};
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) c0[j] = c0[j] + pw[3 * i + j];
    for (int j = 0; j < 3; j++) c0[j] = c0[j] / (double)n;
    double S[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
    for (int i = 0; i < n; i++) {
        const double d[3] = {pw[3 * i] - c0[0], pw[3 * i + 1] - c0[1], pw[3 * i + 2] - c0[2]};
        for (int r = 0; r < 3; r++)
            for (int c = r; c < 3; c++) S[3 * r + c] = S[3 * r + c] + d[r] * d[c];
    }
    S[3] = S[1]; S[6] = S[2]; S[7] = S[5];
    double lam[3], E[9];
    pnp_eig3(S, lam, E);
    for (int j = 0; j < 3; j++) cws[j] = c0[j];
    for (int k = 0; k < 3; k++) {
        // the axis's sign: its largest |component| (the first of equals) is made positive.  With noisy image points EPnP's
        // answer depends on the signs of the control axes, so they are not left to the decomposition
        int big = 0;
        for (int j = 1; j < 3; j++) if (fabs(E[3 * j + k]) > fabs(E[3 * big + k])) big = j;
        if (E[3 * big + k] < 0) for (int j = 0; j < 3; j++) E[3 * j + k] = -E[3 * j + k];
        const double f = sqrt(lam[k] / (double)n);
        for (int j = 0; j < 3; j++) cws[3 * (k + 1) + j] = c0[j] + f * E[3 * j + k];
    }
    double CC[9], ci[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) CC[3 * i + j] = cws[3 * (j + 1) + i] - c0[i];
    if (!pnp_inv3(CC, ci)) return false;
    for (int i = 0; i < n; i++) {
        const double d[3] = {pw[3 * i] - c0[0], pw[3 * i + 1] - c0[1], pw[3 * i + 2] - c0[2]};
        double* a = alphas + 4 * i;
        for (int j = 0; j < 3; j++) a[1 + j] = ci[3 * j] * d[0] + ci[3 * j + 1] * d[1] + ci[3 * j + 2] * d[2];
        a[0] = 1. - a[1] - a[2] - a[3];
    }
    return true;
}

// fill_M: rows 2i, 2i + 1 of M [2n][12]
LVI_PNP_HD void pnp_fill_m(const double* alphas, const double* uv, int n, double* M)
{
    for (int i = 0; i < n; i++) {
        double* m1 = M + 24 * i;
        double* m2 = m1 + 12;
        for (int j = 0; j < 4; j++) {
            const double a = alphas[4 * i + j];
            m1[3 * j] = a; m1[3 * j + 1] = 0.; m1[3 * j + 2] = -(a * uv[2 * i]);
            m2[3 * j] = 0.; m2[3 * j + 1] = a; m2[3 * j + 2] = -(a * uv[2 * i + 1]);
        }
    }
}

// entry (i, j) of M'M, rows summed in order
LVI_PNP_HD double pnp_mtm(const double* M, int rows, int i, int j)
{
    double s = 0.;
    for (int r = 0; r < rows; r++) s = s + M[12 * r + i] * M[12 * r + j];
    return s;
}

// compute_L_6x10 and compute_rho: v4 [4][12], cws [4][3] -> L [6][10], rho [6]
LVI_PNP_HD void pnp_l_rho(const double* v4, const double* cws, double* L, double* rho)
{
    int a = 0, b = 1;
    for (int pr = 0; pr < 6; pr++) {
        double dv[4][3];
        for (int k = 0; k < 4; k++)
            for (int j = 0; j < 3; j++) dv[k][j] = v4[12 * k + 3 * a + j] - v4[12 * k + 3 * b + j];
        auto dot = [&](int x, int y) { return dv[x][0] * dv[y][0] + dv[x][1] * dv[y][1] + dv[x][2] * dv[y][2]; };
        double* l = L + 10 * pr;
        l[0] = dot(0, 0); l[1] = 2. * dot(0, 1); l[2] = dot(1, 1); l[3] = 2. * dot(0, 2); l[4] = 2. * dot(1, 2); l[5] = dot(2, 2);
        l[6] = 2. * dot(0, 3); l[7] = 2. * dot(1, 3); l[8] = 2. * dot(2, 3); l[9] = dot(3, 3);
        const double d[3] = {cws[3 * a] - cws[3 * b], cws[3 * a + 1] - cws[3 * b + 1], cws[3 * a + 2] - cws[3 * b + 2]};
        rho[pr] = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        b++;
        if (b > 3) { a++; b = a + 1; }
    }
}

// find_betas_approx_1 / _2 / _3 (N = 1, 2, 3)
LVI_PNP_HD void pnp_beta_init(int N, const double* L, const double* rho, double* be)
{
    double r[6], x[5] = {0., 0., 0., 0., 0.};
    for (int i = 0; i < 6; i++) r[i] = rho[i];
    if (N == 1) {
        double A[24];
        for (int i = 0; i < 6; i++) { A[4 * i] = L[10 * i]; A[4 * i + 1] = L[10 * i + 1]; A[4 * i + 2] = L[10 * i + 3]; A[4 * i + 3] = L[10 * i + 6]; }
        pnp_lstsq<4>(A, r, x);
        if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = -x[1] / be[0]; be[2] = -x[2] / be[0]; be[3] = -x[3] / be[0]; }
        else { be[0] = sqrt(x[0]); be[1] = x[1] / be[0]; be[2] = x[2] / be[0]; be[3] = x[3] / be[0]; }
        return;
    }
    if (N == 2) {
        double A[18];
        for (int i = 0; i < 6; i++) for (int j = 0; j < 3; j++) A[3 * i + j] = L[10 * i + j];
        pnp_lstsq<3>(A, r, x);
    } else {
        double A[30];
        for (int i = 0; i < 6; i++) for (int j = 0; j < 5; j++) A[5 * i + j] = L[10 * i + j];
        pnp_lstsq<5>(A, r, x);
    }
    if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = x[2] < 0 ? sqrt(-x[2]) : 0.; }
    else { be[0] = sqrt(x[0]); be[1] = x[2] > 0 ? sqrt(x[2]) : 0.; }
    if (x[1] < 0) be[0] = -be[0];
    be[2] = N == 3 ? x[3] / be[0] : 0.;
    be[3] = 0.;
}

// gauss_newton: exactly PNP_GN_STEPS steps
LVI_PNP_HD void pnp_gauss_newton(const double* L, const double* rho, double* be)
{
    for (int it = 0; it < PNP_GN_STEPS; it++) {
        double A[24], r[6], x[4];
        for (int i = 0; i < 6; i++) {
            const double* l = L + 10 * i;
            A[4 * i] = 2. * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3];
            A[4 * i + 1] = l[1] * be[0] + 2. * l[2] * be[1] + l[4] * be[2] + l[7] * be[3];
            A[4 * i + 2] = l[3] * be[0] + l[4] * be[1] + 2. * l[5] * be[2] + l[8] * be[3];
            A[4 * i + 3] = l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2. * l[9] * be[3];
            r[i] = rho[i] - (l[0] * be[0] * be[0] + l[1] * be[0] * be[1] + l[2] * be[1] * be[1] + l[3] * be[0] * be[2] + l[4] * be[1] * be[2] +
                            l[5] * be[2] * be[2] + l[6] * be[0] * be[3] + l[7] * be[1] * be[3] + l[8] * be[2] * be[3] + l[9] * be[3] * be[3]);
        }
        pnp_lstsq<4>(A, r, x);
        for (int k = 0; k < 4; k++) be[k] = be[k] + x[k];
    }
}

// compute_R_and_t: compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error.
// pcs [n][3] is scratch.  Returns the mean reprojection error.
LVI_PNP_HD double pnp_pose(const double* be, const double* v4, const double* alphas, const double* pw, const double* uv, int n, double* pcs, double* R,
                           double* t)
{
    double ccs[12];
    for (int i = 0; i < 12; i++) ccs[i] = 0.;
    for (int k = 0; k < 4; k++)
        for (int j = 0; j < 12; j++) ccs[j] = ccs[j] + be[k] * v4[12 * k + j];
    for (int i = 0; i < n; i++) {
        const double* a = alphas + 4 * i;
        for (int c = 0; c < 3; c++) pcs[3 * i + c] = a[0] * ccs[c] + a[1] * ccs[3 + c] + a[2] * ccs[6 + c] + a[3] * ccs[9 + c];
    }
    if (pcs[2] < 0)
        for (int i = 0; i < 3 * n; i++) pcs[i] = -pcs[i];
    double pc0[3] = {0., 0., 0.}, pw0[3] = {0., 0., 0.};
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) { pc0[j] = pc0[j] + pcs[3 * i + j]; pw0[j] = pw0[j] + pw[3 * i + j]; }
    for (int j = 0; j < 3; j++) { pc0[j] = pc0[j] / (double)n; pw0[j] = pw0[j] / (double)n; }
    double AB[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++) AB[3 * j + k] = AB[3 * j + k] + (pcs[3 * i + j] - pc0[j]) * (pw[3 * i + k] - pw0[k]);
    pnp_polar3(AB, R);
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
    for (int i = 0; i < 3; i++) t[i] = pc0[i] - (R[3 * i] * pw0[0] + R[3 * i + 1] * pw0[1] + R[3 * i + 2] * pw0[2]);
    double sum = 0.;
    for (int i = 0; i < n; i++) {
        const double* p = pw + 3 * i;
        const double xc = R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + t[0];
        const double yc = R[3] * p[0] + R[4] * p[1] + R[5] * p[2] + t[1];
        const double iz = 1. / (R[6] * p[0] + R[7] * p[1] + R[8] * p[2] + t[2]);
        const double du = uv[2 * i] - xc * iz, dv = uv[2 * i + 1] - yc * iz;
        sum = sum + sqrt(du * du + dv * dv);
    }
    return sum / (double)n;
}

// one beta candidate (N = 1, 2, 3): initialisation, refinement, pose -> the reprojection error
LVI_PNP_HD double pnp_candidate(int N, const double* L, const double* rho, const double* v4, const double* alphas, const double* pw, const double* uv, int n,
                                double* pcs, double* R, double* t)
{
    double be[4];
    pnp_beta_init(N, L, rho, be);
    pnp_gauss_newton(L, rho, be);
    return pnp_pose(be, v4, alphas, pw, uv, n, pcs, R, t);
}

// compute_pose's choice among rep[1..3]: a NaN never wins a comparison it enters
LVI_PNP_HD int pnp_choose(const double* rep)
{
    int N = 1;
    if (rep[2] < rep[1]) N = 2;
    if (rep[3] < rep[N]) N = 3;
    return N;
}

// PnPRansacCallback::computeError -> projectPoints with K = I and no distortion
LVI_PNP_HD float pnp_error(const double* R, const double* t, float x, float y, float z, float u, float v)
{
    const double X = R[0] * x + R[1] * y + R[2] * z + t[0];
    const double Y = R[3] * x + R[4] * y + R[5] * z + t[1];
    const double Z = R[6] * x + R[7] * y + R[8] * z + t[2];
    const double iz = Z != 0 ? 1. / Z : 1.;
    const float pu = (float)(X * iz), pv = (float)(Y * iz);
    const float dx = u - pu, dy = v - pv;
    const float dx2 = dx * dx, dy2 = dy * dy;
    return dx2 + dy2;
}

}  // namespace lvi_pnp_math
