// Arithmetic of the feature table (include/lvi_fman.h), shared by the kernels of lvi_fman.hip and by host
// code: it compiles alone with a C++17 host compiler (tests/test_fman_ref.py builds it into a stand-alone program, plain
// and under the host sanitizers).  Every sum is written out term by term, left to right, and the library is built with
// -ffp-contract=off: apart from the triangulated depth the results are the bits tests/fman_ref.py gives.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define LVI_FMAN_HD __host__ __device__ inline
#else
#define LVI_FMAN_HD inline
#endif

namespace lvi_fman_math {

constexpr int WINDOW = 10;          // WINDOW_SIZE
constexpr int MAX_OBS = 11;
constexpr int OBS_DOUBLES = 9;      // point 0..2, uv 3..4, velocity 5..6, depth 7, cur_td 8
constexpr int MAX_ROWS = 2 * MAX_OBS;
constexpr int MAX_SWEEPS = 30;
constexpr double SVD_EPS = 2.220446049250313e-16;   // 2^-52

struct Poses { double Ps[MAX_OBS][3]; double Rs[MAX_OBS][9]; double tic[3]; double ric[9]; };

// std::max / std::min as the library states them: a NaN second argument never wins
LVI_FMAN_HD double max_std(double a, double b) { return (a < b) ? b : a; }
LVI_FMAN_HD double min_std(double a, double b) { return (b < a) ? b : a; }

// getFeatureCount's rule (feature_manager.cpp:36)
LVI_FMAN_HD bool eligible(int n_obs, int start_frame) { return n_obs >= 2 && start_frame < WINDOW - 2; }

// row-major 3 x 3: C = A B, C = A' B, y = A x, y = A' x; every entry (t0 + t1) + t2
LVI_FMAN_HD void mul33(const double* A, const double* B, double* C)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
LVI_FMAN_HD void mul33t(const double* A, const double* B, double* C)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
LVI_FMAN_HD void mul3v(const double* A, const double* x, double* y)
{
    for (int i = 0; i < 3; i++) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2];
}
LVI_FMAN_HD void mul3tv(const double* A, const double* x, double* y)
{
    for (int i = 0; i < 3; i++) y[i] = A[i] * x[0] + A[3 + i] * x[1] + A[6 + i] * x[2];
}

// compensatedParallax2 (:381-414) as written, p_i_comp = p_i and all: p_i, p_j are the points of frames frame_count - 2 and - 1
LVI_FMAN_HD double compensated_parallax2(const double* p_i, const double* p_j)
{
    double ans = 0;
    const double u_j = p_j[0], v_j = p_j[1];
    const double dep_i = p_i[2];
    const double u_i = p_i[0] / dep_i, v_i = p_i[1] / dep_i;
    const double du = u_i - u_j, dv = v_i - v_j;
    const double dep_i_comp = p_i[2];
    const double u_i_comp = p_i[0] / dep_i_comp, v_i_comp = p_i[1] / dep_i_comp;
    const double du_comp = u_i_comp - u_j, dv_comp = v_i_comp - v_j;
    ans = max_std(ans, std::sqrt(min_std(du * du + dv * dv, du_comp * du_comp + dv_comp * dv_comp)));
    return ans;
}

// dep_j of removeBackShiftDepth (:314-317): the old first observation at `depth`, carried into the new first frame
LVI_FMAN_HD double shifted_depth(const double* uv_i, double depth, const double* marg_R, const double* marg_P, const double* new_R, const double* new_P)
{
    const double pts_i[3] = {uv_i[0] * depth, uv_i[1] * depth, uv_i[2] * depth};
    double w[3];
    mul3v(marg_R, pts_i, w);
    const double d[3] = {(w[0] + marg_P[0]) - new_P[0], (w[1] + marg_P[1]) - new_P[1], (w[2] + marg_P[2]) - new_P[2]};
    return new_R[2] * d[0] + new_R[5] * d[1] + new_R[8] * d[2];
}

// the 2k x 4 matrix of triangulate (:223-252); obs: k observations of OBS_DOUBLES doubles, the first at frame `start`
LVI_FMAN_HD void triangulation_rows(const Poses& W, int start, int k, const double* obs, double (*A)[4])
{
    double t0[3], R0[9], v[3];
    mul3v(W.Rs[start], W.tic, v);
    for (int c = 0; c < 3; c++) t0[c] = W.Ps[start][c] + v[c];
    mul33(W.Rs[start], W.ric, R0);
    for (int o = 0; o < k; o++) {
        const int j = start + o;
        double t1[3], R1[9], d[3], t[3], R[9], P[3][4];
        mul3v(W.Rs[j], W.tic, v);
        for (int c = 0; c < 3; c++) t1[c] = W.Ps[j][c] + v[c];
        mul33(W.Rs[j], W.ric, R1);
        for (int c = 0; c < 3; c++) d[c] = t1[c] - t0[c];
        mul3tv(R0, d, t);                                  // t = R0' (t1 - t0)
        mul33t(R0, R1, R);                                 // R = R0' R1
        double Rt_t[3];
        mul3tv(R, t, Rt_t);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) P[r][c] = R[3 * c + r];   // P.leftCols<3>() = R'
            P[r][3] = -Rt_t[r];                                // P.rightCols<1>() = -R' t
        }
        const double* p = obs + o * OBS_DOUBLES;
        const double z = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
        double f[3] = {p[0], p[1], p[2]};
        if (z > 0) { const double n = std::sqrt(z); f[0] = p[0] / n; f[1] = p[1] / n; f[2] = p[2] / n; }   // Eigen's normalized()
        for (int c = 0; c < 4; c++) {
            A[2 * o][c] = f[0] * P[2][c] - f[2] * P[0][c];
            A[2 * o + 1][c] = f[1] * P[2][c] - f[2] * P[1][c];
        }
    }
}

// One-sided (Hestenes) Jacobi SVD of the rows x 4 matrix A, on A itself: A V = U S column by column, so the small singular
// values keep their relative accuracy (A'A is never formed).  Sweep order: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  A pair is
// rotated when |a_p . a_q| > 2^-52 sqrt(|a_p|^2 |a_q|^2).  Stop rule: the first sweep that rotates no pair, or MAX_SWEEPS
// sweeps.  v: the column of V whose |A v|^2 is smallest (the last of equals, as a descending sort leaves it).  Returns the
// sweeps taken.  A is overwritten.
LVI_FMAN_HD int svd_null_vector(double (*A)[4], int rows, double* v)
{
    double V[4][4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
    int sweeps = 0;
    for (; sweeps < MAX_SWEEPS;) {
        sweeps++;
        int rotated = 0;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int r = 0; r < rows; r++) {
                    alpha = alpha + A[r][p] * A[r][p];
                    beta = beta + A[r][q] * A[r][q];
                    gamma = gamma + A[r][p] * A[r][q];
                }
                if (!(std::fabs(gamma) > SVD_EPS * std::sqrt(alpha * beta))) continue;
                rotated++;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double root = std::sqrt(1.0 + zeta * zeta);
                const double t = zeta < 0 ? -1.0 / (-zeta + root) : 1.0 / (zeta + root);
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < rows; r++) {
                    const double ap = A[r][p], aq = A[r][q];
                    A[r][p] = c * ap - s * aq;
                    A[r][q] = s * ap + c * aq;
                }
                for (int r = 0; r < 4; r++) {
                    const double vp = V[r][p], vq = V[r][q];
                    V[r][p] = c * vp - s * vq;
                    V[r][q] = s * vp + c * vq;
                }
            }
        if (rotated == 0) break;
    }
    int best = 0;
    double least = 0;
    for (int c = 0; c < 4; c++) {
        double n2 = 0;
        for (int r = 0; r < rows; r++) n2 = n2 + A[r][c] * A[r][c];
        if (c == 0 || n2 <= least) { least = n2; best = c; }
    }
    for (int r = 0; r < 4; r++) v[r] = V[r][best];
    return sweeps;
}

// svd_method of :254-255, before the sign rule of :262-265
LVI_FMAN_HD double triangulate_depth(const Poses& W, int start, int k, const double* obs, int* sweeps)
{
    double A[MAX_ROWS][4], v[4];
    triangulation_rows(W, start, k, obs, A);
    const int s = svd_null_vector(A, 2 * k, v);
    if (sweeps) *sweeps = s;
    return v[2] / v[3];
}

}  // namespace lvi_fman_math
