// Arithmetic of the initial two-view pose (include/lvi_relpose.h), shared by the kernels of lvi_relpose.hip and
// by host code: it compiles alone with a C++17 host compiler (tests/test_relpose_ref.py builds it into a stand-alone
// program, plain and under the host sanitizers).  A restatement of OpenCV 4.5.x cv::recoverPose / decomposeEssentialMat
// (calib3d/src/five-point.cpp) and triangulatePoints (triangulate.cpp) as MotionEstimator::solveRelativeRT calls them
// (solve_5pts.cpp:193-227): the camera matrix is the identity and the points are cv::Point2f.  Only + - * / sqrt, fabs and
// comparisons; every sum is written out term by term, left to right, and the library is built with -ffp-contract=off: the
// results are the bits tests/relpose_ref.py gives.
#pragma once
#include <cmath>

#include "lvi_fman_math.hpp"

#if defined(__HIPCC__)
#define LVI_RELPOSE_HD __host__ __device__ inline
#else
#define LVI_RELPOSE_HD inline
#endif

namespace lvi_relpose_math {

namespace fm = lvi_fman_math;

constexpr int CANDIDATES = 4;
constexpr double DBL_MAX_ = 1.7976931348623157e308;
constexpr int FLAG_DEGENERATE = 1;   // LVI_RELPOSE_DEGENERATE

// decomposeEssentialMat: R1, R2 row-major, t, the singular values descending
struct Decomp { double R1[9], R2[9], t[3], sv[3]; int degenerate, sweeps; };

LVI_RELPOSE_HD double det33(const double* A)
{
    return (A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6])) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// The SVD of E (rank 2) with all three columns of U defined: one-sided (Hestenes) Jacobi on the columns of B = E', so the
// accumulated rotations are U itself.  Sweep order (0,1) (0,2) (1,2); pair threshold and stop rule of
// lvi_fman_math::svd_null_vector.  Then w_k = E' u_k, sigma_k = |w_k|, sorted descending with the first of equals first,
// v_k = w_k / sigma_k for the two largest and v_3 = v_1 x v_2.  A non-finite entry of E, a non-finite sigma or a second
// sigma that is exactly 0 is no pose: identity, zero, `degenerate` set.
LVI_RELPOSE_HD void decompose(const double* E, Decomp& D)
{
    for (int k = 0; k < 9; k++) { D.R1[k] = D.R2[k] = (k % 4 == 0) ? 1.0 : 0.0; }
    for (int k = 0; k < 3; k++) D.t[k] = D.sv[k] = 0.0;
    D.degenerate = 1; D.sweeps = 0;
    for (int k = 0; k < 9; k++)
        if (!(std::fabs(E[k]) <= DBL_MAX_)) return;
    double B[3][3], J[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { B[r][c] = E[3 * c + r]; J[r][c] = r == c ? 1.0 : 0.0; }
    int sweeps = 0;
    for (; sweeps < fm::MAX_SWEEPS;) {
        sweeps++;
        int rotated = 0;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int r = 0; r < 3; r++) {
                    alpha = alpha + B[r][p] * B[r][p];
                    beta = beta + B[r][q] * B[r][q];
                    gamma = gamma + B[r][p] * B[r][q];
                }
                if (!(std::fabs(gamma) > fm::SVD_EPS * std::sqrt(alpha * beta))) continue;
                rotated++;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double root = std::sqrt(1.0 + zeta * zeta);
                const double t = zeta < 0 ? -1.0 / (-zeta + root) : 1.0 / (zeta + root);
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < 3; r++) {
                    const double bp = B[r][p], bq = B[r][q];
                    B[r][p] = c * bp - s * bq;
                    B[r][q] = s * bp + c * bq;
                    const double jp = J[r][p], jq = J[r][q];
                    J[r][p] = c * jp - s * jq;
                    J[r][q] = s * jp + c * jq;
                }
            }
        if (rotated == 0) break;
    }
    D.sweeps = sweeps;
    // w_k = E' u_k from E itself and the finished U: the rotated columns of B are not used again
    double w[3][3], sig[3];
    for (int k = 0; k < 3; k++) {
        for (int i = 0; i < 3; i++) w[k][i] = (E[i] * J[0][k] + E[3 + i] * J[1][k]) + E[6 + i] * J[2][k];
        sig[k] = std::sqrt((w[k][0] * w[k][0] + w[k][1] * w[k][1]) + w[k][2] * w[k][2]);
    }
    int ord[3] = {0, 1, 2};
    for (int i = 1; i < 3; i++)                                   // insertion sort, descending, stable
        for (int j = i; j > 0 && sig[ord[j]] > sig[ord[j - 1]]; j--) { const int x = ord[j]; ord[j] = ord[j - 1]; ord[j - 1] = x; }
    const double s0 = sig[ord[0]], s1 = sig[ord[1]], s2 = sig[ord[2]];
    if (!(s0 <= DBL_MAX_) || !(s1 > 0.0)) return;
    double U[9], Vt[9];
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) U[3 * r + k] = J[r][ord[k]];
    for (int i = 0; i < 3; i++) { Vt[i] = w[ord[0]][i] / s0; Vt[3 + i] = w[ord[1]][i] / s1; }
    Vt[6] = Vt[1] * Vt[5] - Vt[2] * Vt[4];
    Vt[7] = Vt[2] * Vt[3] - Vt[0] * Vt[5];
    Vt[8] = Vt[0] * Vt[4] - Vt[1] * Vt[3];
    if (det33(U) < 0)
        for (int k = 0; k < 9; k++) U[k] = -U[k];
    if (det33(Vt) < 0)
        for (int k = 0; k < 9; k++) Vt[k] = -Vt[k];
    double UW[9], UWt[9];                                          // U W and U W', W = [0 1 0; -1 0 0; 0 0 1]
    for (int r = 0; r < 3; r++) {
        UW[3 * r] = -U[3 * r + 1]; UW[3 * r + 1] = U[3 * r]; UW[3 * r + 2] = U[3 * r + 2];
        UWt[3 * r] = U[3 * r + 1]; UWt[3 * r + 1] = -U[3 * r]; UWt[3 * r + 2] = U[3 * r + 2];
    }
    fm::mul33(UW, Vt, D.R1);
    fm::mul33(UWt, Vt, D.R2);
    for (int r = 0; r < 3; r++) D.t[r] = U[3 * r + 2];
    D.sv[0] = s0; D.sv[1] = s1; D.sv[2] = s2;
    D.degenerate = 0;
}

// candidate c of recoverPose in OpenCV's order: [R1|t], [R2|t], [R1|-t], [R2|-t] -> P row-major 3 x 4
LVI_RELPOSE_HD void candidate(const Decomp& D, int c, double (*P)[4])
{
    const double* R = (c & 1) ? D.R2 : D.R1;
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) P[r][k] = R[3 * r + k];
        P[r][3] = c >= 2 ? -D.t[r] : D.t[r];
    }
}

// One point under one candidate: triangulatePoints of (x1, y1) under P0 = [I|0] and (x2, y2) under P, then the masks of
// recoverPose: Q2 Q3 > 0, z < dist, z' > 0, z' < dist.  A Q3 of zero makes every comparison false as IEEE gives them.
LVI_RELPOSE_HD int cheirality(const double (*P)[4], double x1, double y1, double x2, double y2, double dist)
{
    const double P0[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
    double A[4][4], Q[4];
    for (int k = 0; k < 4; k++) {
        A[0][k] = x1 * P0[2][k] - P0[0][k];
        A[1][k] = y1 * P0[2][k] - P0[1][k];
        A[2][k] = x2 * P[2][k] - P[0][k];
        A[3][k] = y2 * P[2][k] - P[1][k];
    }
    fm::svd_null_vector(A, 4, Q);
    int m = Q[2] * Q[3] > 0;
    const double X = Q[0] / Q[3], Y = Q[1] / Q[3], Z = Q[2] / Q[3], W = Q[3] / Q[3];
    m = m && (Z < dist);
    const double z2 = ((P[2][0] * X + P[2][1] * Y) + P[2][2] * Z) + P[2][3] * W;
    m = m && (z2 > 0);
    m = m && (z2 < dist);
    return m ? 1 : 0;
}

// the first candidate in OpenCV's order whose count is >= the three others
LVI_RELPOSE_HD int choose(const int* good)
{
    for (int c = 0; c < CANDIDATES; c++) {
        int best = 1;
        for (int o = 0; o < CANDIDATES; o++) best = best && good[c] >= good[o];
        if (best) return c;
    }
    return CANDIDATES - 1;
}

// lvi_relpose_pose, field for field
struct Pose { double R[9], t[3], sv[3]; int good[CANDIDATES], chosen, n_inliers, flags, sweeps; };

// cand [c]: R row-major, then t
LVI_RELPOSE_HD void candidate_record(const Decomp& D, int c, double* cand)
{
    double P[3][4];
    candidate(D, c, P);
    for (int r = 0; r < 3; r++) {
        for (int j = 0; j < 3; j++) cand[3 * r + j] = P[r][j];
        cand[9 + r] = P[r][3];
    }
}

// what recoverPose returns, from the decomposition and the four counts
LVI_RELPOSE_HD void fill_pose(const Decomp& D, const int* good, Pose& o)
{
    const int ch = choose(good);
    double cand[12];
    candidate_record(D, ch, cand);
    for (int j = 0; j < 9; j++) o.R[j] = cand[j];
    for (int j = 0; j < 3; j++) { o.t[j] = cand[9 + j]; o.sv[j] = D.sv[j]; }
    for (int c = 0; c < CANDIDATES; c++) o.good[c] = good[c];
    o.chosen = ch; o.n_inliers = good[ch];
    o.flags = D.degenerate ? FLAG_DEGENERATE : 0;
    o.sweeps = D.sweeps;
}

// cv::recoverPose on one thread: pts [n][4] = x1 y1 x2 y2, in_mask [n] or null (all ones), masks [4][n] receives 0 / 1
LVI_RELPOSE_HD void recover_serial(const double* E, const float* pts, const unsigned char* in_mask, int n, double dist, Pose& o, double (*cand)[12],
                                   unsigned char* masks)
{
    Decomp D;
    decompose(E, D);
    int good[CANDIDATES];
    for (int c = 0; c < CANDIDATES; c++) {
        double P[3][4];
        candidate(D, c, P);
        candidate_record(D, c, cand[c]);
        good[c] = 0;
        for (int k = 0; k < n; k++) {
            int bit = 0;
            if (!D.degenerate)
                bit = cheirality(P, (double)pts[4 * k], (double)pts[4 * k + 1], (double)pts[4 * k + 2], (double)pts[4 * k + 3], dist) && (!in_mask || in_mask[k] != 0);
            masks[(long)c * n + k] = (unsigned char)bit;
            good[c] += bit;
        }
    }
    fill_pose(D, good, o);
}

// Rotation = R', Translation = -R' T (solve_5pts.cpp:219-220), every entry (t0 + t1) + t2
LVI_RELPOSE_HD void invert_pose(const double* R, const double* T, double* Rotation, double* Translation)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Rotation[3 * i + j] = R[3 * j + i];
        Translation[i] = ((-R[i]) * T[0] + (-R[3 + i]) * T[1]) + (-R[6 + i]) * T[2];
    }
}

// average_parallax of Estimator::relativePose (estimator.cpp:502-512) over pairs [n][6] (first xyz, second xyz), on the doubles
LVI_RELPOSE_HD double average_parallax(const double* pairs, int n)
{
    double sum_parallax = 0;
    for (int j = 0; j < n; j++) {
        const double dx = pairs[6 * j] - pairs[6 * j + 3], dy = pairs[6 * j + 1] - pairs[6 * j + 4];
        sum_parallax = sum_parallax + std::sqrt(dx * dx + dy * dy);
    }
    return 1.0 * sum_parallax / n;
}

}  // namespace lvi_relpose_math
