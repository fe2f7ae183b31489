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
//
// The batched handle (include/lvi_fmatb.h) runs the same two bodies for up to LVI_TRACKER_MAX_BATCH point sets
// on one stream: fmatb_hyp once per active slot, enqueued while the host draws the next slot's stream, then fmatb_walk once
// with one wave per slot, one download and one wait.
#include <chrono>
#include <cfloat>
#include <cmath>

#include "lvi_ransac.hpp"
#include "../../include/lvi_fmatb.h"   // includes lvi_fmat.h

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

// One hypothesis of one point-pair set (workgroup h of the set's launch): the body of fmat_hyp and fmatb_hyp
__device__ __forceinline__ void hyp_body(const HypArgs& a, int h)
{
    extern __shared__ float4 sp[];                             // the n correspondences
    __shared__ double sa[7 * 9];                               // the 7x9 system
    __shared__ double sF[27];
    __shared__ int s_piv[7], s_r, s_c, s_nm;
    __shared__ unsigned s_err[64];
    const int lane = threadIdx.x;
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

__global__ __launch_bounds__(LVI_WAVE) void fmat_hyp(HypArgs a) { hyp_body(a, blockIdx.x); }
// a slot of lvi_fmatb_find: the same body on the slot's regions of the handle's buffers, one launch per active slot
__global__ __launch_bounds__(LVI_WAVE) void fmatb_hyp(HypArgs a) { hyp_body(a, blockIdx.x); }

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

// The walk and the status of one point-pair set by one wave: the body of fmat_walk and fmatb_walk
__device__ __forceinline__ void walk_body(const WalkArgs& a)
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

__global__ __launch_bounds__(LVI_WAVE) void fmat_walk(WalkArgs a) { walk_body(a); }

// The scalars of a slot's WalkArgs: the record at the head of the slot's input region, uploaded with the slot's points
struct WalkRec {
    int n, nsub, path, niters0;
    double num_log;
    float thr;
};

// What the slots of a batched handle share: the two blocks, the per-hypothesis arrays of all slots and the strides that
// lead to slot s's part of each.  The record holds no pointer: a pointer read from memory has no known address space and
// every load through it would be a flat load; pointers built from these kernel arguments load as fmat_walk's do.
struct WalkBatch {
    const char* d_in;       // [S] x (WalkRec | pts | subsets | logtab)
    char* d_out;            // [S] x (info | status)
    const double* F;        // [S][I][27]
    const int* nmodels;     // [S][I]
    const int* score;       // [S][I][3]
    size_t in_stride, off_set, off_log, out_stride, off_status;
    int I;
    unsigned active;        // bit s: slot s takes part in this call
};

// All slots of lvi_fmatb_find in one launch: workgroup s walks slot s; a slot that sits out returns at once
__global__ __launch_bounds__(LVI_WAVE) void fmatb_walk(WalkBatch b)
{
    const size_t s = blockIdx.x;
    if (!((b.active >> s) & 1u)) return;
    const char* in = b.d_in + b.in_stride * s;
    char* out = b.d_out + b.out_stride * s;
    const WalkRec r = *reinterpret_cast<const WalkRec*>(in);
    const WalkArgs a{reinterpret_cast<const float4*>(in + b.off_set), reinterpret_cast<const double*>(in + b.off_set + b.off_log),
                     b.F + 27 * (size_t)b.I * s, b.nmodels + (size_t)b.I * s, b.score + 3 * (size_t)b.I * s,
                     r.n, r.nsub, r.path, r.niters0, r.num_log, r.thr,
                     reinterpret_cast<lvi_fmat_info*>(out), reinterpret_cast<unsigned char*>(out + b.off_status)};
    walk_body(a);
}

// ---------------------------------------------------------------------------------------------- host: one point set
// the input region of one point set: pts [P] float4 | subsets [I][7] | logtab [P + 1]; its output region: info | status [P]
struct Layout {
    size_t off_sub = 0, off_log = 0, in_bytes = 0, off_status = 0, out_bytes = 0;
    void set(int P, int I)
    {
        off_sub = align256(sizeof(float4) * (size_t)P);
        off_log = off_sub + align256(sizeof(int) * 7 * (size_t)I);
        in_bytes = off_log + align256(sizeof(double) * ((size_t)P + 1));
        off_status = align256(sizeof(lvi_fmat_info));
        out_bytes = off_status + align256((size_t)P);
    }
};

// what the host half of a call leaves in a point set's input region
struct Staged {
    int n, path, nsub, niters0;
    float thr;              // (float)(threshold * threshold)
    double num_log;
    double stream_us;
    size_t up;              // bytes of the region to upload: the points, then (if any) the subsets and the log table
};

// findFundamentalMat's argument defaults, the interleaved points, the path rule, the sample stream and the log table
Staged stage_set(char* h_in, const Layout& L, int I, int check, const float* pts1_xy, const float* pts2_xy, int n, double threshold, double confidence, Trace& tr)
{
    if (threshold <= 0) threshold = 3;
    if (confidence < DBL_EPSILON || confidence > 1 - DBL_EPSILON) confidence = 0.99;
    float* xy = reinterpret_cast<float*>(h_in);
    for (int i = 0; i < n; i++) {
        xy[4 * i] = pts1_xy[2 * i]; xy[4 * i + 1] = pts1_xy[2 * i + 1];
        xy[4 * i + 2] = pts2_xy[2 * i]; xy[4 * i + 3] = pts2_xy[2 * i + 1];
    }
    int* sub = reinterpret_cast<int*>(h_in + L.off_sub);
    double* lt = reinterpret_cast<double*>(h_in + L.off_log);
    Staged g{};
    g.n = n;
    g.path = n == MODEL_POINTS ? LVI_FMAT_PATH_KERNEL : n < 15 ? LVI_FMAT_PATH_LMEDS : LVI_FMAT_PATH_RANSAC;
    const auto t0 = std::chrono::steady_clock::now();
    g.nsub = 1; g.niters0 = 1;
    if (g.path == LVI_FMAT_PATH_KERNEL) {
        for (int k = 0; k < MODEL_POINTS; k++) sub[k] = k;
    } else {
        g.nsub = fm_sample_stream(xy, n, g.path == LVI_FMAT_PATH_RANSAC, I, confidence, check, sub, &g.niters0);
        if (g.path == LVI_FMAT_PATH_RANSAC) for (int k = 0; k <= n; k++) lt[k] = update_log<MODEL_POINTS>(n, k);
    }
    g.stream_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    tr.record(sub, MODEL_POINTS, g.nsub);
    g.thr = (float)(threshold * threshold);
    g.num_log = num_log(confidence);
    g.up = g.path == LVI_FMAT_PATH_RANSAC ? L.off_log + sizeof(double) * (n + 1) : L.off_sub + sizeof(int) * 7 * (size_t)g.nsub;
    return g;
}

// the per-hypothesis arrays of one point set
struct HypBufs {
    double* F = nullptr;                   // [I][27]
    int *nm = nullptr, *score = nullptr;   // [I], [I][3]
    template <class A> void carve(A& a, size_t I) { F = a.template alloc<double>(27 * I); nm = a.template alloc<int>(I); score = a.template alloc<int>(3 * I); }
};

HypArgs hyp_args(const Staged& g, const Layout& L, const char* d_in, const HypBufs& b)
{
    return HypArgs{reinterpret_cast<const float4*>(d_in), reinterpret_cast<const int*>(d_in + L.off_sub), g.n, g.path == LVI_FMAT_PATH_LMEDS ? 1 : 0, g.thr, b.F, b.nm, b.score};
}

WalkArgs walk_args(const Staged& g, const Layout& L, const char* d_in, const HypBufs& b, char* d_out)
{
    return WalkArgs{reinterpret_cast<const float4*>(d_in), reinterpret_cast<const double*>(d_in + L.off_log), b.F, b.nm, b.score, g.n, g.nsub, g.path, g.niters0, g.num_log, g.thr,
                    reinterpret_cast<lvi_fmat_info*>(d_out), reinterpret_cast<unsigned char*>(d_out + L.off_status)};
}

// the device half of a trace: the first m hypotheses of one point set, one wait
void trace_hyp(hipStream_t stream, const HypBufs& b, int m, int32_t* nmodels, double* F, int32_t* score)
{
    if (nmodels) LVI_HIP(hipMemcpyAsync(nmodels, b.nm, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, stream));
    if (F) LVI_HIP(hipMemcpyAsync(F, b.F, sizeof(double) * 27 * (size_t)m, hipMemcpyDeviceToHost, stream));
    if (score) LVI_HIP(hipMemcpyAsync(score, b.score, sizeof(int) * 3 * (size_t)m, hipMemcpyDeviceToHost, stream));
    LVI_HIP(hipStreamSynchronize(stream));
}

}  // namespace

// ---------------------------------------------------------------------------------------------- the handle
struct lvi_fmat {
    int P = 0, I = 0, check = 1;
    Io io;
    Layout L;
    HypBufs hb;
};

extern "C" {

int32_t lvi_fmat_abi_version(void) { return LVI_FMAT_ABI_VERSION; }

int32_t lvi_fmat_create(int32_t device, int32_t max_points, int32_t max_iters, lvi_fmat** out)
{
    if (!out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (max_points < MODEL_POINTS || max_points > LVI_FMAT_MAX_POINTS) return fail(LVI_ERR_INVALID_ARG, "max_points must be 7..LVI_FMAT_MAX_POINTS");
    if (max_iters < 1 || max_iters > LVI_FMAT_MAX_ITERS) return fail(LVI_ERR_INVALID_ARG, "max_iters must be 1..LVI_FMAT_MAX_ITERS");
    return create_handle(device, out, lvi_fmat_destroy,
        [&](lvi_fmat* h) { h->P = max_points; h->I = max_iters; h->L.set(h->P, h->I); },
        [&](lvi_fmat* h) -> int32_t { h->io.open(device, h->L.in_bytes, h->L.out_bytes, [&](auto& a) { h->hb.carve(a, (size_t)h->I); }); return LVI_OK; });
}

void lvi_fmat_destroy(lvi_fmat* h)
{
    if (!h) return;
    h->io.close();
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
        const Staged g = stage_set(io.h_in, h->L, h->I, h->check, pts1_xy, pts2_xy, n, threshold, confidence, io);
        io.run(g.up, n, g.stream_us, status_out, info_out, [&](lvi_fmat_info*, unsigned char*) {
            if (g.nsub > 0) {
                hipLaunchKernelGGL(fmat_hyp, dim3(g.nsub), dim3(LVI_WAVE), sizeof(float4) * (size_t)n, io.stream, hyp_args(g, h->L, io.d_in, h->hb));
                LVI_HIP(hipGetLastError());
            }
            hipLaunchKernelGGL(fmat_walk, dim3(1), dim3(LVI_WAVE), 0, io.stream, walk_args(g, h->L, io.d_in, h->hb, io.d_out));
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
        if (m > 0) trace_hyp(h->io.stream, h->hb, m, nmodels, F, score);
        return LVI_OK;
    });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- the batched handle
// include/lvi_fmatb.h, DESIGN §25: `slots` point sets per call on one stream.  Slot s owns a region of each block:
//   d_in / h_in    [s * in_stride]   the slot's WalkRec | the region of a single handle (Layout)
//   d_out / h_out  [s * L.out_bytes] info | status [P]
// and slot s's part [s * I] of each per-hypothesis array, so no slot reads what another wrote.
struct lvi_fmatb {
    int S = 0, P = 0, I = 0, check = 1;
    Bufs io;
    Layout L;
    size_t off_set = 0, in_stride = 0;     // the slot's Layout region starts off_set bytes into the slot's input region
    HypBufs hb;                            // [S][I]...
    Trace tr[LVI_TRACKER_MAX_BATCH];
    int64_t calls = 0, hyp_launches = 0, walk_launches = 0, waits = 0;
    HypBufs slot(int s) const { return HypBufs{hb.F + 27 * (size_t)I * s, hb.nm + (size_t)I * s, hb.score + 3 * (size_t)I * s}; }
};

extern "C" {

int32_t lvi_fmatb_abi_version(void) { return LVI_FMATB_ABI_VERSION; }

int32_t lvi_fmatb_create(int32_t device, int32_t slots, int32_t max_points, int32_t max_iters, lvi_fmatb** out)
{
    if (!out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (slots < 1 || slots > LVI_TRACKER_MAX_BATCH) return fail(LVI_ERR_INVALID_ARG, "slots must be 1..LVI_TRACKER_MAX_BATCH");
    if (max_points < MODEL_POINTS || max_points > LVI_FMAT_MAX_POINTS) return fail(LVI_ERR_INVALID_ARG, "max_points must be 7..LVI_FMAT_MAX_POINTS");
    if (max_iters < 1 || max_iters > LVI_FMAT_MAX_ITERS) return fail(LVI_ERR_INVALID_ARG, "max_iters must be 1..LVI_FMAT_MAX_ITERS");
    return create_handle(device, out, lvi_fmatb_destroy, [&](lvi_fmatb* h) {
        h->S = slots; h->P = max_points; h->I = max_iters;
        h->L.set(h->P, h->I);
        h->off_set = align256(sizeof(WalkRec));
        h->in_stride = h->off_set + h->L.in_bytes;
    }, [&](lvi_fmatb* h) -> int32_t {
        h->io.open(device, h->in_stride * (size_t)slots, h->L.out_bytes * (size_t)slots, [&](auto& a) { h->hb.carve(a, (size_t)slots * (size_t)h->I); });
        return LVI_OK;
    });
}

void lvi_fmatb_destroy(lvi_fmatb* h)
{
    if (!h) return;
    h->io.close();
    delete h;
}

int32_t lvi_fmatb_set_check_subset(lvi_fmatb* h, int32_t mode)
{
    if (!h || (mode != 0 && mode != 1)) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    h->check = mode;
    return LVI_OK;
}

int32_t lvi_fmatb_find(lvi_fmatb* h, const float* const* pts1_xy, const float* const* pts2_xy, const int32_t* n, const double* threshold, double confidence,
                       uint8_t* const* status_out, lvi_fmat_info* info_out)
{
    if (!h || !pts1_xy || !pts2_xy || !n || !threshold || !status_out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    // every slot's arguments before anything is written, staged or launched
    unsigned active = 0;
    for (int s = 0; s < h->S; s++) {
        if (n[s] == -1) continue;
        if (!pts1_xy[s] || !pts2_xy[s] || !status_out[s]) return fail(LVI_ERR_INVALID_ARG, "null argument in an active slot");
        if (n[s] < MODEL_POINTS) return fail(LVI_ERR_INVALID_ARG, "n < 7 in a slot (-1 = the slot sits out): findFundamentalMat has no model");
        if (n[s] > h->P) return fail(LVI_ERR_INVALID_ARG, "n > max_points in a slot");
        active |= 1u << s;
    }
    Bufs& io = h->io;
    return guarded(io.device, [&]() -> int32_t {
        for (int s = 0; s < h->S; s++) if (!((active >> s) & 1u)) {
            h->tr[s].clear();
            if (info_out) std::memset(&info_out[s], 0, sizeof(lvi_fmat_info));
        }
        if (!active) return LVI_OK;
        double stream_us[LVI_TRACKER_MAX_BATCH] = {};
        // per active slot: the host's half, then the slot's upload and its hypotheses enqueued; the device scores slot s
        // while the host draws the stream of slot s + 1
        for (int s = 0; s < h->S; s++) {
            if (!((active >> s) & 1u)) continue;
            char* hs = io.h_in + h->in_stride * (size_t)s;
            const char* ds = io.d_in + h->in_stride * (size_t)s;
            const Staged g = stage_set(hs + h->off_set, h->L, h->I, h->check, pts1_xy[s], pts2_xy[s], n[s], threshold[s], confidence, h->tr[s]);
            stream_us[s] = g.stream_us;
            const WalkRec rec{g.n, g.nsub, g.path, g.niters0, g.num_log, g.thr};
            std::memcpy(hs, &rec, sizeof(WalkRec));
            LVI_HIP(hipMemcpyAsync(io.d_in + h->in_stride * (size_t)s, hs, h->off_set + g.up, hipMemcpyHostToDevice, io.stream));
            if (g.nsub > 0) {
                hipLaunchKernelGGL(fmatb_hyp, dim3(g.nsub), dim3(LVI_WAVE), sizeof(float4) * (size_t)g.n, io.stream, hyp_args(g, h->L, ds + h->off_set, h->slot(s)));
                LVI_HIP(hipGetLastError());
                h->hyp_launches++;
            }
        }
        const WalkBatch wb{io.d_in, io.d_out, h->hb.F, h->hb.nm, h->hb.score, h->in_stride, h->off_set, h->L.off_log, h->L.out_bytes, h->L.off_status, h->I, active};
        hipLaunchKernelGGL(fmatb_walk, dim3(h->S), dim3(LVI_WAVE), 0, io.stream, wb);
        LVI_HIP(hipGetLastError());
        h->walk_launches++;
        LVI_HIP(hipMemcpyAsync(io.h_out, io.d_out, h->L.out_bytes * (size_t)h->S, hipMemcpyDeviceToHost, io.stream));
        LVI_HIP(hipStreamSynchronize(io.stream));
        h->waits++;
        h->calls++;
        for (int s = 0; s < h->S; s++) {
            if (!((active >> s) & 1u)) continue;
            const char* o = io.h_out + h->L.out_bytes * (size_t)s;
            std::memcpy(status_out[s], o + h->L.off_status, (size_t)n[s]);
            if (info_out) {
                std::memcpy(&info_out[s], o, sizeof(lvi_fmat_info));
                info_out[s].stream_us = stream_us[s];
            }
        }
        return LVI_OK;
    });
}

int32_t lvi_fmatb_trace(lvi_fmatb* h, int32_t slot, int32_t* subsets, int32_t* nmodels, double* F, int32_t* score, int32_t cap, int32_t* n_out)
{
    if (!h || cap < 0 || slot < 0 || slot >= h->S) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    return guarded(h->io.device, [&]() -> int32_t {
        const int m = h->tr[slot].trace_subsets(subsets, MODEL_POINTS, cap, n_out);
        if (m > 0) trace_hyp(h->io.stream, h->slot(slot), m, nmodels, F, score);
        return LVI_OK;
    });
}

int32_t lvi_fmatb_counters(lvi_fmatb* h, int64_t* calls, int64_t* hyp_launches, int64_t* walk_launches, int64_t* waits)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (calls) *calls = h->calls;
    if (hyp_launches) *hyp_launches = h->hyp_launches;
    if (walk_launches) *walk_launches = h->walk_launches;
    if (waits) *waits = h->waits;
    return LVI_OK;
}

}  // extern "C"

