// KeyFrame::PnPRANSAC's cv::solvePnPRansac(matched_3d, matched_2d_old_norm, K = I, D, rvec, t, true, 100, 10.0 / 460.0,
// 0.99, inliers) on the GPU (keyframe.cpp:135-176; include/lvi_pnp.h; the contract is DESIGN §16).
//
//   host       the sample stream: getSubset with modelPoints = 5 (lvi_ransac.hpp).  The PnP callback has no checkSubset,
//              so the first five distinct draws are the subset and getSubset never fails
//   pnp_hyp    one wave per hypothesis: EPnP on the subset's five points (epnp.cpp compute_pose, lvi_pnp_math.hpp) in
//              double — the 12x12 eigenproblem by round-robin Jacobi with its entries spread over the lanes, the three
//              beta candidates on three lanes — then every lane scores the n points against the chosen pose
//   pnp_walk   one wave replays the sequential RANSAC walk (lvi_ransac.hpp) from the counts and writes the chosen
//              hypothesis's status
//
// Everything scored is double with -ffp-contract=off; only sqrt and division come from the math library (both IEEE-exact
// in f64), so for the same (R, t) bits the errors are those of the host restatement.
#include <chrono>
#include <cfloat>
#include <cmath>

#include "lvi_ransac.hpp"
#include "lvi_pnp_math.hpp"
#include "../../include/lvi_pnp.h"

using namespace lvi;
using namespace lvi_pnp_math;
using namespace lvi_ransac;

namespace {

constexpr int MODEL_POINTS = 5;
constexpr int LD = 13;                       // row stride of the 12x12 matrices in LDS: a column walk (stride 26 banks) hits 12 distinct bank pairs

struct HypArgs {
    const float* p3;        // [n][3]
    const float* p2;        // [n][2]
    const int* subsets;     // [nsub][5]
    int n;
    float thr;              // (float)((double)thr * thr) of the float parameter
    double* Rt;             // [nsub][12]
    int* has;               // [nsub]
    int* good;              // [nsub]
    int* wb;                // [nsub]
};

__global__ __launch_bounds__(LVI_WAVE) void pnp_hyp(HypArgs a)
{
    __shared__ double s_pw[15], s_uv[10], s_cws[12], s_al[20], s_M[120];
    __shared__ double s_A[12 * LD], s_V[12 * LD], s_cs[12];
    __shared__ double s_v4[48], s_L[60], s_rho[6];
    __shared__ double s_R[3][9], s_t[3][3], s_rep[4], s_pcs[3][15];
    __shared__ int s_ok, s_N, s_idx[4];
    const int h = blockIdx.x, lane = threadIdx.x;
    if (lane < MODEL_POINTS) {
        const int i = a.subsets[MODEL_POINTS * h + lane];
        for (int j = 0; j < 3; j++) s_pw[3 * lane + j] = (double)a.p3[3 * i + j];
        for (int j = 0; j < 2; j++) s_uv[2 * lane + j] = (double)a.p2[2 * i + j];
    }
    __syncthreads();
    if (lane == 0) {
        const bool ok = pnp_control_points(s_pw, MODEL_POINTS, s_cws, s_al);
        if (ok) pnp_fill_m(s_al, s_uv, MODEL_POINTS, s_M);
        s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (!s_ok) {                                               // uniform: an exactly singular control-point matrix, no model
        if (lane < 12) a.Rt[12 * (size_t)h + lane] = 0.;
        if (lane == 0) { a.has[h] = 0; a.good[h] = 0; a.wb[h] = 0; }
        return;
    }
    // M'M and V = I, entry e of the 144 on lane e % 64
    for (int e = lane; e < 144; e += LVI_WAVE) {
        const int i = e / 12, j = e % 12;
        s_A[LD * i + j] = pnp_mtm(s_M, 2 * MODEL_POINTS, i, j);
        s_V[LD * i + j] = i == j ? 1. : 0.;
    }
    __syncthreads();
    for (int sw = 0; sw < PNP_SWEEPS12; sw++)
        for (int r = 0; r < 11; r++) {
            if (lane < 6) {
                int p, q;
                double c, s;
                jacobi12_pair(r, lane, &p, &q);
                pnp_rot(s_A[LD * p + q], s_A[LD * p + p], s_A[LD * q + q], &c, &s);
                s_cs[2 * lane] = c; s_cs[2 * lane + 1] = s;
            }
            __syncthreads();
            double na[3], nv[3];
            for (int k = 0; k < 3; k++) {
                const int e = lane + LVI_WAVE * k;
                if (e < 144) na[k] = jacobi12_row(s_A, LD, s_cs, r, e / 12, e % 12);
            }
            __syncthreads();
            for (int k = 0; k < 3; k++) {
                const int e = lane + LVI_WAVE * k;
                if (e < 144) s_A[LD * (e / 12) + e % 12] = na[k];
            }
            __syncthreads();
            for (int k = 0; k < 3; k++) {
                const int e = lane + LVI_WAVE * k;
                if (e < 144) {
                    na[k] = jacobi12_col(s_A, LD, s_cs, r, e / 12, e % 12);
                    nv[k] = jacobi12_col(s_V, LD, s_cs, r, e / 12, e % 12);
                }
            }
            __syncthreads();
            for (int k = 0; k < 3; k++) {
                const int e = lane + LVI_WAVE * k;
                if (e < 144) { s_A[LD * (e / 12) + e % 12] = na[k]; s_V[LD * (e / 12) + e % 12] = nv[k]; }
            }
            __syncthreads();
        }
    if (lane == 0) {
        double lam[12];
        int idx[4];
        for (int i = 0; i < 12; i++) lam[i] = s_A[LD * i + i];
        pnp_smallest4(lam, idx);
        for (int k = 0; k < 4; k++) s_idx[k] = idx[k];
    }
    __syncthreads();
    if (lane < 48) s_v4[lane] = s_V[LD * (lane % 12) + s_idx[lane / 12]];
    __syncthreads();
    if (lane == 0) pnp_l_rho(s_v4, s_cws, s_L, s_rho);
    __syncthreads();
    if (lane < 3) s_rep[lane + 1] = pnp_candidate(lane + 1, s_L, s_rho, s_v4, s_al, s_pw, s_uv, MODEL_POINTS, s_pcs[lane], s_R[lane], s_t[lane]);
    __syncthreads();
    if (lane == 0) s_N = pnp_choose(s_rep);
    __syncthreads();
    const int N = s_N;
    double R[9], t[3];
    for (int k = 0; k < 9; k++) R[k] = s_R[N - 1][k];
    for (int k = 0; k < 3; k++) t[k] = s_t[N - 1][k];
    int good = 0;
    for (int base = 0; base < a.n; base += LVI_WAVE) {
        const int i = base + lane;
        const bool in = i < a.n && pnp_error(R, t, a.p3[3 * i], a.p3[3 * i + 1], a.p3[3 * i + 2], a.p2[2 * i], a.p2[2 * i + 1]) <= a.thr;
        good += __popcll(__ballot(in));
    }
    if (lane < 9) a.Rt[12 * (size_t)h + lane] = R[lane];
    else if (lane < 12) a.Rt[12 * (size_t)h + lane] = t[lane - 9];
    if (lane == 0) { a.has[h] = 1; a.good[h] = good; a.wb[h] = N; }
}

struct WalkArgs {
    const float* p3;
    const float* p2;
    const double* logtab;   // [n + 1] log(1 - (1 - ep)^5) per inlier count, +inf = denom < DBL_MIN
    const double* Rt;
    const int* has;
    const int* good;
    const int* wb;
    int n, nsub, path, niters0;
    double num_log;         // log(max(1 - confidence, DBL_MIN))
    float thr;
    lvi_pnp_info* info;
    unsigned char* status;
};

__global__ __launch_bounds__(LVI_WAVE) void pnp_walk(WalkArgs a)
{
    __shared__ int s_best;
    const int lane = threadIdx.x;
    if (lane == 0) {
        Walk w{1, -1, -1};                                     // the direct path: one iteration
        if (a.path == LVI_PNP_PATH_DIRECT) {
            if (a.nsub > 0 && a.has[0]) w.best_iter = 0;
        } else {
            w = ransac_walk<MODEL_POINTS>(a.has, a.good, 1, a.nsub, a.niters0, a.num_log, a.logtab);   // has: 0 or 1 model per hypothesis
        }
        const int best = w.best_iter;
        s_best = best;
        lvi_pnp_info* o = a.info;
        o->path = a.path; o->iters = w.iter; o->n_subsets = a.nsub; o->best_iter = best;
        o->which_beta = best >= 0 ? a.wb[best] : 0;
        for (int k = 0; k < 9; k++) o->R[k] = best >= 0 ? a.Rt[12 * (size_t)best + k] : 0.;
        for (int k = 0; k < 3; k++) o->t[k] = best >= 0 ? a.Rt[12 * (size_t)best + 9 + k] : 0.;
        o->stream_us = 0.;
    }
    __syncthreads();
    const int best = s_best;
    double R[9], t[3];
    for (int k = 0; k < 9; k++) R[k] = best >= 0 ? a.Rt[12 * (size_t)best + k] : 0.;
    for (int k = 0; k < 3; k++) t[k] = best >= 0 ? a.Rt[12 * (size_t)best + 9 + k] : 0.;
    const int good = status_sweep(a.n, a.status, [&](int i) {
        if (best < 0) return false;
        return a.path == LVI_PNP_PATH_DIRECT ? true : pnp_error(R, t, a.p3[3 * i], a.p3[3 * i + 1], a.p3[3 * i + 2], a.p2[2 * i], a.p2[2 * i + 1]) <= a.thr;
    });
    if (lane == 0) a.info->n_inliers = good;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- the handle
struct lvi_pnp {
    int P = 0, I = 0;
    Io io;                                 // d_in: pts3d [P][3] | pts2d [P][2] | subsets [I][5] | logtab [P + 1]; d_out: info | status [P]
    double* d_Rt = nullptr;                // [I][12]
    int *d_has = nullptr, *d_good = nullptr, *d_wb = nullptr;
    size_t off_p2 = 0, off_sub = 0, off_log = 0;
};

extern "C" {

int32_t lvi_pnp_abi_version(void) { return LVI_PNP_ABI_VERSION; }

int32_t lvi_pnp_create(int32_t device, int32_t max_points, int32_t max_iters, lvi_pnp** out)
{
    if (!out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (max_points < MODEL_POINTS || max_points > LVI_PNP_MAX_POINTS) return fail(LVI_ERR_INVALID_ARG, "max_points must be 5..LVI_PNP_MAX_POINTS");
    if (max_iters < 1 || max_iters > LVI_PNP_MAX_ITERS) return fail(LVI_ERR_INVALID_ARG, "max_iters must be 1..LVI_PNP_MAX_ITERS");
    return create_handle(device, out, lvi_pnp_destroy, [&](lvi_pnp* h) {
        h->P = max_points; h->I = max_iters;
        h->off_p2 = align256(sizeof(float) * 3 * (size_t)h->P);
        h->off_sub = h->off_p2 + align256(sizeof(float) * 2 * (size_t)h->P);
        h->off_log = h->off_sub + align256(sizeof(int) * MODEL_POINTS * (size_t)h->I);
    }, [&](lvi_pnp* h) -> int32_t {
        h->io.open(device, h->off_log + align256(sizeof(double) * ((size_t)h->P + 1)), align256(sizeof(lvi_pnp_info)) + align256((size_t)h->P), [&](auto& a) {
            const size_t I = (size_t)h->I;
            h->d_Rt = a.template alloc<double>(12 * I); h->d_has = a.template alloc<int>(I); h->d_good = a.template alloc<int>(I); h->d_wb = a.template alloc<int>(I);
        });
        return LVI_OK;
    });
}

void lvi_pnp_destroy(lvi_pnp* h)
{
    if (!h) return;
    h->io.close();
    delete h;
}

int32_t lvi_pnp_solve(lvi_pnp* h, const float* pts3d_xyz, const float* pts2d_xy, int32_t n, double threshold, double confidence, uint8_t* status_out,
                      lvi_pnp_info* info_out)
{
    if (!h || !pts3d_xyz || !pts2d_xy || !status_out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (n < MODEL_POINTS) return fail(LVI_ERR_INVALID_ARG, "n < 5: the P3P path of solvePnPRansac is not restated");
    if (n > h->P) return fail(LVI_ERR_INVALID_ARG, "n > max_points");
    Io& io = h->io;
    return guarded(io.device, [&]() -> int32_t {
        std::memcpy(io.h_in, pts3d_xyz, sizeof(float) * 3 * (size_t)n);
        std::memcpy(io.h_in + h->off_p2, pts2d_xy, sizeof(float) * 2 * (size_t)n);
        int* sub = reinterpret_cast<int*>(io.h_in + h->off_sub);
        double* lt = reinterpret_cast<double*>(io.h_in + h->off_log);
        const int path = n == MODEL_POINTS ? LVI_PNP_PATH_DIRECT : LVI_PNP_PATH_RANSAC;
        const auto t0 = std::chrono::steady_clock::now();
        int nsub = 1;
        if (path == LVI_PNP_PATH_DIRECT) {
            for (int k = 0; k < MODEL_POINTS; k++) sub[k] = k;
            for (int g = 0; g <= n; g++) lt[g] = 0.;                   // the walk does not read the table on this path
        } else {
            nsub = sample_stream<MODEL_POINTS>(n, h->I, 1, [](const int32_t*) { return true; }, sub);
            for (int g = 0; g <= n; g++) lt[g] = update_log<MODEL_POINTS>(n, g);
        }
        const double stream_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        io.record(sub, MODEL_POINTS, nsub);

        const float thr_param = (float)threshold;                      // solvePnPRansac's `float reprojectionError`
        const float thr = (float)((double)thr_param * thr_param);
        // one upload: points, subsets, and the log table
        io.run(h->off_log + sizeof(double) * ((size_t)n + 1), n, stream_us, status_out, info_out, [&](lvi_pnp_info* d_info, unsigned char* d_status) {
            const float* d_p3 = reinterpret_cast<const float*>(io.d_in);
            const float* d_p2 = reinterpret_cast<const float*>(io.d_in + h->off_p2);
            HypArgs ha{d_p3, d_p2, reinterpret_cast<const int*>(io.d_in + h->off_sub), n, thr, h->d_Rt, h->d_has, h->d_good, h->d_wb};
            hipLaunchKernelGGL(pnp_hyp, dim3(nsub), dim3(LVI_WAVE), 0, io.stream, ha);
            LVI_HIP(hipGetLastError());
            WalkArgs wa{d_p3, d_p2, reinterpret_cast<const double*>(io.d_in + h->off_log), h->d_Rt, h->d_has, h->d_good, h->d_wb, n, nsub, path, h->I, num_log(confidence), thr,
                        d_info, d_status};
            hipLaunchKernelGGL(pnp_walk, dim3(1), dim3(LVI_WAVE), 0, io.stream, wa);
            LVI_HIP(hipGetLastError());
        });
        return LVI_OK;
    });
}

int32_t lvi_pnp_trace(lvi_pnp* h, int32_t* subsets, int32_t* has_model, double* Rt, int32_t* good, int32_t cap, int32_t* n_out)
{
    if (!h || cap < 0) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    return guarded(h->io.device, [&]() -> int32_t {
        const int m = h->io.trace_subsets(subsets, MODEL_POINTS, cap, n_out);
        if (m == 0) return LVI_OK;
        if (has_model) LVI_HIP(hipMemcpyAsync(has_model, h->d_has, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, h->io.stream));
        if (Rt) LVI_HIP(hipMemcpyAsync(Rt, h->d_Rt, sizeof(double) * 12 * (size_t)m, hipMemcpyDeviceToHost, h->io.stream));
        if (good) LVI_HIP(hipMemcpyAsync(good, h->d_good, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, h->io.stream));
        LVI_HIP(hipStreamSynchronize(h->io.stream));
        return LVI_OK;
    });
}

}  // extern "C"
