// rejectWithF's cv::findFundamentalMat(un_cur, un_forw, FM_RANSAC, F_THRESHOLD, 0.99, status) on the GPU
// (feature_tracker.cpp:209-242; include/lvi_fmat.h; the contract is DESIGN §11).
//
//   host       the sample stream: getSubset with the FM callback's checkSubset (lvi_ransac.hpp)
//   fmat_hyp   one wave per hypothesis: the 7-point kernel (fundam.cpp run7Point, with a Gauss-Jordan null space) in
//              double, then every lane scores the 1..3 candidates over the points held in LDS
//   fmat_walk  one wave replays the sequential RANSAC (lvi_ransac.hpp) or LMeDS (LMeDSPointSetRegistrator::run) walk
//              from the counts / medians and writes the chosen model's status
//
// Everything scored is double with -ffp-contract=off: for the same F bits the errors are those of the host restatement.
#include <chrono>
#include <cfloat>
#include <cmath>

#include "lvi_ransac.hpp"
#include "../../include/lvi_fmat.h"

using namespace lvi;
using namespace lvi_ransac;

namespace {

constexpr int MODEL_POINTS = FM_MODEL_POINTS;

// ---------------------------------------------------------------------------------------------- device
struct HypArgs {
    const float4* pts;      // (x1, y1, x2, y2) per correspondence
    const int* subsets;     // [nsub][7]
    int n, lmeds;
    float thr;              // RANSAC: (float)(threshold * threshold)
    double* F;              // [nsub][3][9]
    int* nmodels;           // [nsub]
    int* score;             // [nsub][3]: inlier count (RANSAC) or median f32 bits (LMeDS)
};

// FMEstimatorCallback::computeError: err = (float)max(d1^2 s1, d2^2 s2)
__device__ __forceinline__ float fm_err(const double* F, float4 p)
{
    const double x1 = p.x, y1 = p.y, x2 = p.z, y2 = p.w;
    double a = F[0] * x1 + F[1] * y1 + F[2];
    double b = F[3] * x1 + F[4] * y1 + F[5];
    double c = F[6] * x1 + F[7] * y1 + F[8];
    const double s2 = 1. / (a * a + b * b);
    const double d2 = x2 * a + y2 * b + c;
    a = F[0] * x2 + F[3] * y2 + F[6];
    b = F[1] * x2 + F[4] * y2 + F[7];
    c = F[2] * x2 + F[5] * y2 + F[8];
    const double s1 = 1. / (a * a + b * b);
    const double d1 = x1 * a + y1 * b + c;
    const double e1 = d1 * d1 * s1, e2 = d2 * d2 * s2;
    return (float)(e1 < e2 ? e2 : e1);                         // std::max(e1, e2)
}

// cv::solveCubic (mathfuncs.cpp) for coefficients c[0..3] of c0 x^3 + c1 x^2 + c2 x + c3
__device__ int solve_cubic(const double* c, double* r)
{
    int n = 0;
    double a0 = c[0], a1 = c[1], a2 = c[2], a3 = c[3];
    double x0 = 0., x1 = 0., x2 = 0.;
    if (a0 == 0) {
        if (a1 == 0) {
            if (a2 == 0) n = a3 == 0 ? -1 : 0;
            else { x0 = -a3 / a2; n = 1; }
        } else {
            double d = a2 * a2 - 4 * a1 * a3;
            if (d >= 0) {
                d = sqrt(d);
                const double q1 = (-a2 + d) * 0.5, q2 = (a2 + d) * -0.5;
                if (fabs(q1) > fabs(q2)) { x0 = q1 / a1; x1 = a3 / q1; }
                else { x0 = q2 / a1; x1 = a3 / q2; }
                n = d > 0 ? 2 : 1;
            }
        }
    } else {
        a0 = 1. / a0;
        a1 *= a0; a2 *= a0; a3 *= a0;
        const double Q = (a1 * a1 - 3 * a2) * (1. / 9);
        const double R = (a1 * (2 * a1 * a1 - 9 * a2) + 27 * a3) * (1. / 54);
        const double Qcubed = Q * Q * Q;
        double d = (a1 * a1 * (a2 * a2 - 4 * a1 * a3) + 2 * a2 * (9 * a1 * a3 - 2 * a2 * a2) - 27 * a3 * a3) * (1. / 108);
        if (d > 0) {
            const double theta = acos(R / sqrt(Qcubed));
            const double sqrtQ = sqrt(Q);
            const double t0 = -2 * sqrtQ, t1 = theta * (1. / 3);
            const double twoPiThird = 2.0943951023931954923084289221863;
            x0 = t0 * cos(t1) - a1 * (1. / 3);
            x1 = t0 * cos(t1 + twoPiThird) - a1 * (1. / 3);
            x2 = t0 * cos(t1 - twoPiThird) - a1 * (1. / 3);
            n = 3;
        } else if (d == 0) {
            if (R >= 0) { x0 = -2 * pow(R, 1. / 3) - a1 / 3; x1 = pow(R, 1. / 3) - a1 / 3; }
            else { x0 = 2 * pow(-R, 1. / 3) - a1 / 3; x1 = -pow(-R, 1. / 3) - a1 / 3; }
            x2 = 0;
            n = x0 == x1 ? 1 : 2;
            x1 = x0 == x1 ? 0 : x1;
        } else {
            d = sqrt(-d);
            double e = pow(d + fabs(R), 1. / 3);
            if (R > 0) e = -e;
            x0 = (e + Q / e) - a1 * (1. / 3);
            n = 1;
        }
    }
    r[0] = x0; r[1] = x1; r[2] = x2;
    return n;
}

// run7Point's cubic and per-root normalisation (fundam.cpp), from the null-space basis f1, f2 (f1 is modified)
__device__ int seven_point_roots(double* f1, const double* f2, double* F)
{
    double c[4], r[3];
    for (int i = 0; i < 9; i++) f1[i] -= f2[i];
    double t0 = f2[4] * f2[8] - f2[5] * f2[7];
    double t1 = f2[3] * f2[8] - f2[5] * f2[6];
    double t2 = f2[3] * f2[7] - f2[4] * f2[6];
    c[3] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2;
    c[2] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2 -
           f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) +
           f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) -
           f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) +
           f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) -
           f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
           f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]);
    t0 = f1[4] * f1[8] - f1[5] * f1[7];
    t1 = f1[3] * f1[8] - f1[5] * f1[6];
    t2 = f1[3] * f1[7] - f1[4] * f1[6];
    c[1] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2 -
           f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) +
           f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) -
           f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) +
           f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) -
           f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
           f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]);
    c[0] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2;
    const int n = solve_cubic(c, r);
    if (n < 1 || n > 3) return 0;                              // run7Point returns n; runKernel's caller skips n <= 0
    for (int k = 0; k < n; k++, F += 9) {
        double lambda = r[k], mu = 1.;
        const double s = f1[8] * r[k] + f2[8];
        if (fabs(s) > DBL_EPSILON) { mu = 1. / s; lambda *= mu; F[8] = 1.; }
        else F[8] = 0.;
        for (int i = 0; i < 8; i++) F[i] = f1[i] * lambda + f2[i] * mu;
    }
    return n;
}

__global__ __launch_bounds__(LVI_WAVE) void fmat_hyp(HypArgs a)
{
    extern __shared__ float4 sp[];                             // the n correspondences
    __shared__ double sa[7 * 9];                               // the 7x9 system
    __shared__ double sF[27];
    __shared__ int s_piv[7], s_r, s_c, s_nm;
    __shared__ unsigned s_err[64];
    const int h = blockIdx.x, lane = threadIdx.x;
    for (int i = lane; i < a.n; i += LVI_WAVE) sp[i] = a.pts[i];
    __syncthreads();
    // rows (x1 x0, x1 y0, x1, y1 x0, y1 y0, y1, x0, y0, 1) of run7Point: (m2, 1)' F (m1, 1) = 0
    if (lane < 7) {
        const float4 p = sp[a.subsets[7 * h + lane]];
        const double x0 = p.x, y0 = p.y, x1 = p.z, y1 = p.w;
        double* row = sa + 9 * lane;
        row[0] = x1 * x0; row[1] = x1 * y0; row[2] = x1; row[3] = y1 * x0; row[4] = y1 * y0; row[5] = y1; row[6] = x0; row[7] = y0; row[8] = 1;
    }
    if (lane == 0) s_r = 0;
    __syncthreads();
    // Gauss-Jordan with partial pivoting, column by column; a column whose largest remaining |entry| is 0 is free
    for (int c = 0; c < 9; c++) {
        if (s_r == 7) break;                                   // uniform: read after a barrier
        if (lane == 0) {
            const int r = s_r;
            int p = r;
            double best = fabs(sa[9 * r + c]);
            for (int i = r + 1; i < 7; i++) if (fabs(sa[9 * i + c]) > best) { best = fabs(sa[9 * i + c]); p = i; }
            if (best == 0) s_c = -1;
            else {
                if (p != r) for (int j = 0; j < 9; j++) { const double t = sa[9 * r + j]; sa[9 * r + j] = sa[9 * p + j]; sa[9 * p + j] = t; }
                s_c = c; s_piv[r] = c;
            }
        }
        __syncthreads();
        if (s_c >= 0) {
            const int r = s_r;
            const int i = lane / 9, j = lane % 9;
            double v = 0.;
            bool wr = false;
            if (lane < 63 && i != r && j >= c) {
                const double f = sa[9 * i + c] / sa[9 * r + c];
                v = j == c ? 0. : sa[9 * i + j] - f * sa[9 * r + j];
                wr = true;
            }
            __syncthreads();
            if (wr) sa[9 * i + j] = v;
            if (lane == 0) s_r = r + 1;
        }
        __syncthreads();
    }
    if (lane == 0) {
        int nm = 0;
        if (s_r == 7) {
            // the two free columns in increasing order; basis vector k: x[free_k] = 1, x[pivot col of row q] = -a[q][free_k] / a[q][q's pivot]
            int fc[2], nf = 0;
            for (int c = 0; c < 9 && nf < 2; c++) {
                bool piv = false;
                for (int q = 0; q < 7; q++) piv |= s_piv[q] == c;
                if (!piv) fc[nf++] = c;
            }
            double f1[9], f2[9];
            for (int j = 0; j < 9; j++) { f1[j] = 0.; f2[j] = 0.; }
            f1[fc[0]] = 1.; f2[fc[1]] = 1.;
            for (int q = 0; q < 7; q++) {
                const double d = sa[9 * q + s_piv[q]];
                f1[s_piv[q]] = -sa[9 * q + fc[0]] / d;
                f2[s_piv[q]] = -sa[9 * q + fc[1]] / d;
            }
            nm = seven_point_roots(f1, f2, sF);
        }
        for (int k = nm * 9; k < 27; k++) sF[k] = 0.;
        s_nm = nm;
        a.nmodels[h] = nm;
        for (int k = 0; k < 27; k++) a.F[27 * (size_t)h + k] = sF[k];
    }
    __syncthreads();
    const int nm = s_nm;
    for (int m = 0; m < 3; m++) {
        int sc = 0;
        if (m < nm && !a.lmeds) {
            for (int base = 0; base < a.n; base += LVI_WAVE) {
                const int i = base + lane;
                const bool in = i < a.n && fm_err(sF + 9 * m, sp[i]) <= a.thr;
                sc += __popcll(__ballot(in));
            }
        } else if (m < nm) {
            // nth_element(err as int, n/2): the element whose stable rank among the int bit patterns is n/2 (n < 15 here)
            if (lane < a.n) s_err[lane] = (unsigned)__float_as_int(fm_err(sF + 9 * m, sp[lane]));
            __syncthreads();
            if (lane < a.n) {
                const int e = (int)s_err[lane];
                int rank = 0;
                for (int j = 0; j < a.n; j++) { const int o = (int)s_err[j]; rank += o < e || (o == e && j < lane); }
                if (rank == a.n / 2) s_nm = e;                 // s_nm is free now; exactly one lane writes
            }
            __syncthreads();
            sc = s_nm;
            __syncthreads();
        }
        if (lane == 0) a.score[3 * h + m] = sc;
    }
}

struct WalkArgs {
    const float4* pts;
    const double* logtab;   // [n + 1] log(1 - (1 - ep)^7) per goodCount, +inf = denom < DBL_MIN
    const double* F;
    const int* nmodels;
    const int* score;
    int n, nsub, path, niters0;
    double num_log;         // log(max(1 - confidence, DBL_MIN))
    float thr;
    lvi_fmat_info* info;
    unsigned char* status;
};

__global__ __launch_bounds__(LVI_WAVE) void fmat_walk(WalkArgs a)
{
    __shared__ int s_best;
    __shared__ float s_thr;
    const int lane = threadIdx.x;
    if (lane == 0) {
        Walk w{0, -1, -1};
        double best_median = 0.;
        float thr = a.thr;
        if (a.path == LVI_FMAT_PATH_KERNEL) {
            w.iter = 1;
            if (a.nmodels[0] > 0) { w.best_iter = 0; w.best_root = 0; }
        } else if (a.path == LVI_FMAT_PATH_RANSAC) {
            w = ransac_walk<MODEL_POINTS>(a.nmodels, a.score, 3, a.nsub, a.niters0, a.num_log, a.logtab);
        } else {                                                // LMeDS
            double min_median = DBL_MAX;
            for (; w.iter < a.niters0; w.iter++) {
                if (w.iter >= a.nsub) break;
                const int nm = a.nmodels[w.iter];
                for (int m = 0; m < nm; m++) {
                    const double median = (double)__int_as_float(a.score[3 * w.iter + m]);
                    if (median < min_median) { min_median = median; w.best_iter = w.iter; w.best_root = m; }
                }
            }
            if (w.best_iter >= 0) {
                best_median = min_median;
                double sigma = 2.5 * 1.4826 * (1 + 5. / (a.n - MODEL_POINTS)) * sqrt(min_median);
                sigma = sigma > 0.001 ? sigma : 0.001;
                thr = (float)(sigma * sigma);
            }
        }
        s_best = w.best_iter >= 0 ? 3 * w.best_iter + w.best_root : -1;
        s_thr = thr;
        lvi_fmat_info* o = a.info;
        o->path = a.path; o->iters = w.iter; o->n_subsets = a.nsub; o->best_iter = w.best_iter; o->best_root = w.best_root;
        o->best_median = best_median;
        for (int k = 0; k < 9; k++) o->F[k] = w.best_iter >= 0 ? a.F[9 * (size_t)s_best + k] : 0.;
    }
    __syncthreads();
    const int best = s_best;
    const float thr = s_thr;
    double F[9];
    for (int k = 0; k < 9; k++) F[k] = best >= 0 ? a.F[9 * (size_t)best + k] : 0.;
    const int good = status_sweep(a.n, a.status, [&](int i) { return a.path == LVI_FMAT_PATH_KERNEL ? true : best >= 0 && fm_err(F, a.pts[i]) <= thr; });
    if (lane == 0) a.info->n_inliers = good;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- the handle
struct lvi_fmat {
    int P = 0, I = 0, check = 1;
    Io io;                                 // d_in: pts [P] float4 | subsets [I][7] | logtab [P + 1]; d_out: info | status [P]
    double* d_F = nullptr;                 // [I][27]
    int *d_nm = nullptr, *d_score = nullptr;
    size_t off_sub = 0, off_log = 0;
};

extern "C" {

int32_t lvi_fmat_abi_version(void) { return LVI_FMAT_ABI_VERSION; }

int32_t lvi_fmat_create(int32_t device, int32_t max_points, int32_t max_iters, lvi_fmat** out)
{
    if (!out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (max_points < MODEL_POINTS || max_points > LVI_FMAT_MAX_POINTS) return fail(LVI_ERR_INVALID_ARG, "max_points must be 7..LVI_FMAT_MAX_POINTS");
    if (max_iters < 1 || max_iters > LVI_FMAT_MAX_ITERS) return fail(LVI_ERR_INVALID_ARG, "max_iters must be 1..LVI_FMAT_MAX_ITERS");
    lvi_fmat* h = new lvi_fmat();
    h->P = max_points; h->I = max_iters;
    h->off_sub = align256(sizeof(float4) * (size_t)h->P);
    h->off_log = h->off_sub + align256(sizeof(int) * 7 * (size_t)h->I);
    const int32_t st = h->io.open(device, h->off_log + align256(sizeof(double) * ((size_t)h->P + 1)), align256(sizeof(lvi_fmat_info)) + align256((size_t)h->P),
                                  {{(void**)&h->d_F, sizeof(double) * 27 * (size_t)h->I},
                                   {(void**)&h->d_nm, sizeof(int) * (size_t)h->I},
                                   {(void**)&h->d_score, sizeof(int) * 3 * (size_t)h->I}});
    if (st != LVI_OK) { lvi_fmat_destroy(h); return st; }
    *out = h;
    return LVI_OK;
}

void lvi_fmat_destroy(lvi_fmat* h)
{
    if (!h) return;
    h->io.close({h->d_F, h->d_nm, h->d_score});
    delete h;
}

int32_t lvi_fmat_set_check_subset(lvi_fmat* h, int32_t mode)
{
    if (!h || (mode != 0 && mode != 1)) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    h->check = mode;
    return LVI_OK;
}

int32_t lvi_fmat_find(lvi_fmat* h, const float* pts1_xy, const float* pts2_xy, int32_t n, double threshold, double confidence,
                      uint8_t* status_out, lvi_fmat_info* info_out)
{
    if (!h || !pts1_xy || !pts2_xy || !status_out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (n < MODEL_POINTS) return fail(LVI_ERR_INVALID_ARG, "n < 7: findFundamentalMat has no model");
    if (n > h->P) return fail(LVI_ERR_INVALID_ARG, "n > max_points");
    Io& io = h->io;
    return guarded(io.device, [&]() -> int32_t {
        // findFundamentalMat's argument defaults
        if (threshold <= 0) threshold = 3;
        if (confidence < DBL_EPSILON || confidence > 1 - DBL_EPSILON) confidence = 0.99;
        float* xy = reinterpret_cast<float*>(io.h_in);
        for (int i = 0; i < n; i++) {
            xy[4 * i] = pts1_xy[2 * i]; xy[4 * i + 1] = pts1_xy[2 * i + 1];
            xy[4 * i + 2] = pts2_xy[2 * i]; xy[4 * i + 3] = pts2_xy[2 * i + 1];
        }
        int* sub = reinterpret_cast<int*>(io.h_in + h->off_sub);
        double* lt = reinterpret_cast<double*>(io.h_in + h->off_log);
        const int path = n == MODEL_POINTS ? LVI_FMAT_PATH_KERNEL : n < 15 ? LVI_FMAT_PATH_LMEDS : LVI_FMAT_PATH_RANSAC;
        const auto t0 = std::chrono::steady_clock::now();
        int nsub = 1, niters0 = 1;
        if (path == LVI_FMAT_PATH_KERNEL) {
            for (int k = 0; k < MODEL_POINTS; k++) sub[k] = k;
        } else {
            nsub = fm_sample_stream(xy, n, path == LVI_FMAT_PATH_RANSAC, h->I, confidence, h->check, sub, &niters0);
            if (path == LVI_FMAT_PATH_RANSAC) for (int g = 0; g <= n; g++) lt[g] = update_log<MODEL_POINTS>(n, g);
        }
        const double stream_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        io.record(sub, MODEL_POINTS, nsub);

        const float thr = (float)(threshold * threshold);
        // one upload: the points, then (if any) the subsets and the log table
        const size_t up = path == LVI_FMAT_PATH_RANSAC ? h->off_log + sizeof(double) * (n + 1) : h->off_sub + sizeof(int) * 7 * (size_t)nsub;
        io.run(up, n, stream_us, status_out, info_out, [&](lvi_fmat_info* d_info, unsigned char* d_status) {
            const float4* d_pts = reinterpret_cast<const float4*>(io.d_in);
            if (nsub > 0) {
                HypArgs ha{d_pts, reinterpret_cast<const int*>(io.d_in + h->off_sub), n, path == LVI_FMAT_PATH_LMEDS ? 1 : 0, thr, h->d_F, h->d_nm, h->d_score};
                hipLaunchKernelGGL(fmat_hyp, dim3(nsub), dim3(LVI_WAVE), sizeof(float4) * (size_t)n, io.stream, ha);
                LVI_HIP(hipGetLastError());
            }
            WalkArgs wa{d_pts, reinterpret_cast<const double*>(io.d_in + h->off_log), h->d_F, h->d_nm, h->d_score, n, nsub, path, niters0, num_log(confidence), thr,
                        d_info, d_status};
            hipLaunchKernelGGL(fmat_walk, dim3(1), dim3(LVI_WAVE), 0, io.stream, wa);
            LVI_HIP(hipGetLastError());
        });
        return LVI_OK;
    });
}

int32_t lvi_fmat_trace(lvi_fmat* h, int32_t* subsets, int32_t* nmodels, double* F, int32_t* score, int32_t cap, int32_t* n_out)
{
    if (!h || cap < 0) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    return guarded(h->io.device, [&]() -> int32_t {
        const int m = h->io.trace_subsets(subsets, MODEL_POINTS, cap, n_out);
        if (m == 0) return LVI_OK;
        if (nmodels) LVI_HIP(hipMemcpyAsync(nmodels, h->d_nm, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, h->io.stream));
        if (F) LVI_HIP(hipMemcpyAsync(F, h->d_F, sizeof(double) * 27 * (size_t)m, hipMemcpyDeviceToHost, h->io.stream));
        if (score) LVI_HIP(hipMemcpyAsync(score, h->d_score, sizeof(int) * 3 * (size_t)m, hipMemcpyDeviceToHost, h->io.stream));
        LVI_HIP(hipStreamSynchronize(h->io.stream));
        return LVI_OK;
    });
}

}  // extern "C"
