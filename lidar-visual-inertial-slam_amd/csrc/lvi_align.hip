// lvi_align.hip — the visual-inertial alignment of vins_estimator's initialisation on the device (include/lvi_align.h,
// DESIGN §31).
//
// Four kernels, plain HIP C++ with vector stores only.
//   align_repropagate  the integration body of lvi_preint_dev.hpp, which describes it, in its form without the covariance,
//                      one workgroup of 256 threads per job.  A push and a fresh pending preintegration are one job that
//                      travels as the kernel argument; the repropagation of a solve is one job per frame, read from the
//                      solve's upload, with the bias the gyro kernel left on the device.
//   align_gyro         one lane per pair computes the pair's nine plus three products, twelve lanes sum them in pair order,
//                      one lane solves the 3 x 3 system and advances Bgs.
//   align_system       one lane per pair builds r_A and r_b; after a barrier one thread per entry of the compact system
//                      gathers its pairs in ascending order onto 0 or the previous pass's system and scales by 1000.
//   align_factor_solve one wavefront works on the band and the border in LDS: the columns are serial, within a column the
//                      at most 5 + 4 rows below the pivot are one lane each; one lane substitutes, applies the gates or the
//                      gravity step and leaves the state for the next launch.  Latency-bound, with almost no parallelism.
// A solve is one upload (Bgs, the parameters, the list's poses and slots), gyro, repropagate, system and solve, four times
// system and solve, and one download; a kernel that finds the reason already set returns at once.
//
// What follows from the caller's own arguments lives on the host: the list (stamps, poses, flags, which slot holds which
// frame, how many samples), acc_0 / gyr_0.  The device holds what the kernels compute.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lvi_align.h"
#include "lvi_align_math.hpp"
#include "lvi_preint_dev.hpp"

using namespace lvi_preint_dev;
namespace am = lvi_align_math;

static_assert(LVI_ALIGN_OK == am::OK && LVI_ALIGN_GRAVITY_NORM == am::GRAVITY_NORM && LVI_ALIGN_NEGATIVE_SCALE == am::NEGATIVE_SCALE &&
              LVI_ALIGN_NEGATIVE_SCALE_REFINED == am::NEGATIVE_SCALE_REFINED && LVI_ALIGN_SINGULAR == am::SINGULAR && LVI_ALIGN_TOO_FEW == am::TOO_FEW &&
              LVI_ALIGN_APPLY_OPPOSITE == am::APPLY_OPPOSITE && LVI_ALIGN_SYSTEMS == am::SYSTEMS, "the codes of lvi_align_math.hpp");
static_assert(sizeof(lvi_align_info) == 16 + 8 * 16, "lvi_align_info layout");
static_assert(sizeof(lvi_align_frame) == 8 * 13 + 16 + 8 * (1 + 3 + 4 + 3 + 3 + 3 + 3 + 3 + 225), "lvi_align_frame layout");

namespace {

constexpr int MAXF = LVI_ALIGN_MAX_FRAMES, MAXND = 3 * MAXF, MAXN = MAXND + am::NB_LINEAR;
constexpr int PAIR_DOUBLES = 110;                             // r_A (at most 10 x 10) and r_b
constexpr int SYS_STRIDE = am::BW * MAXND + (am::NB_LINEAR + 2) * MAXN;

// one frame of the list as a solve uploads it
struct FrameIn {
    double R[9], T[3];
    int32_t phys, count;
};
struct SolveHead {
    double Bgs[33], TIC[3], G[3];
    int32_t F, reserved;
};
// what the chain leaves between its launches and what a solve downloads; x [MAXN] lies behind it
struct Work {
    int32_t reason, n_state, built, reserved;
    double delta_bg[3], s, g_linear[3], g[3], min_pivot[6], Bgs[33], g0[3];
};

__global__ __launch_bounds__(TB) void align_repropagate(Job jb, const FrameIn* __restrict__ fin, const Work* __restrict__ wk, FrameState* __restrict__ states,
                                                        double* __restrict__ smp, int max_samples)
{
    __shared__ double sJ[NN], sF[2][NN], sS[CHUNK * SD];
    __shared__ pm::StepGeom sG[CHUNK];
    if (jb.flags & J_LIST) list_job(jb, fin[blockIdx.x + 1], wk->Bgs);   // :31-35: frame blockIdx.x + 1 of the list with Ba = 0 and the new Bgs[0]
    integrate_job<false>({sJ, sF, sS, sG}, jb, states, smp, max_samples, nullptr, nullptr);
}

__global__ __launch_bounds__(TB) void align_gyro(const SolveHead* __restrict__ head, const FrameIn* __restrict__ fin, const FrameState* __restrict__ states,
                                                 Work* __restrict__ wk)
{
    __shared__ double sP[(MAXF - 1) * 12], sA[12];
    const int tid = threadIdx.x, F = head->F;
    if (tid < F - 1) {
        const FrameState& sj = states[fin[tid + 1].phys];
        am::gyro_pair(fin[tid].R, fin[tid + 1].R, sj.s.delta_q, sj.jacobian, sP + 12 * tid);
    }
    __syncthreads();
    if (tid < 12) {
        double s = 0.;
        for (int p = 0; p < F - 1; p++) s = s + sP[12 * p + tid];
        sA[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double A[9], b[3], mp = 0.;
        for (int k = 0; k < 9; k++) A[k] = sA[k];
        for (int k = 0; k < 3; k++) b[k] = sA[9 + k];
        Work w{};
        w.reason = am::gyro_solve(A, b, w.delta_bg, &mp);
        w.n_state = 3 * F + am::NB_LINEAR;
        w.min_pivot[0] = mp;
        for (int i = 0; i < 11; i++)
            for (int k = 0; k < 3; k++) w.Bgs[3 * i + k] = head->Bgs[3 * i + k] + w.delta_bg[k];
        *wk = w;
    }
}

__global__ __launch_bounds__(TB) void align_system(int which, const SolveHead* __restrict__ head, const FrameIn* __restrict__ fin,
                                                   const FrameState* __restrict__ states, const Work* __restrict__ wk, double* __restrict__ pairs,
                                                   double* __restrict__ sys)
{
    if (wk->reason != am::OK) return;
    const int tid = threadIdx.x, F = head->F, nd = 3 * F, nb = which == 0 ? am::NB_LINEAR : am::NB_REFINE, n = nd + nb, W = 6 + nb;
    double g0[3] = {wk->g0[0], wk->g0[1], wk->g0[2]}, lxly[6];
    if (which >= 1) am::tangent_basis(g0, lxly);
    if (tid < F - 1) {
        const pm::State& sj = states[fin[tid + 1].phys].s;
        am::Pre pre;
        copy_pre(sj, pre);
        double rA[100], rb[10];
        am::pair_system(fin[tid].R, fin[tid].T, fin[tid + 1].R, fin[tid + 1].T, pre, head->TIC, which >= 1 ? lxly : nullptr, g0, rA, rb);
        double* o = pairs + (size_t)PAIR_DOUBLES * tid;
        for (int k = 0; k < W * W; k++) o[k] = rA[k];
        for (int k = 0; k < W; k++) o[100 + k] = rb[k];
    }
    __syncthreads();                                           // the pairs are in global memory and visible to the workgroup
    double* S = sys + (size_t)SYS_STRIDE * which;
    const double* prev = which >= 2 ? S - SYS_STRIDE : nullptr;   // RefineGravity does not clear A and b between its passes
    const int ob = am::off_bord(nd), obb = am::off_b(nd, nb), ox = am::off_x(nd, nb);
    for (int e = tid; e < ox + n; e += TB) {
        if (e >= ox) { S[e] = 0.; continue; }                 // x
        double v = prev ? prev[e] : 0.;
        int row, col = 0;                                      // the entry in the frame of the dense system; of b when is_b
        const bool is_b = e >= obb;
        if (e < ob) { row = e / am::BW; col = row - e % am::BW; }
        else if (!is_b) { row = nd + (e - ob) / n; col = (e - ob) % n; }
        else row = e - obb;
        const bool stored = is_b || (col >= 0 && col <= row);
        if (stored) {
            const int lead = is_b ? row : col;                // the smaller index decides which pairs hold the entry
            int p0, p1;
            if (lead >= nd) { p0 = 0; p1 = F - 2; }
            else { p0 = max(0, lead / 3 - 1); p1 = min(F - 2, lead / 3); }
            for (int p = p0; p <= p1; p++) {
                const double* o = pairs + (size_t)PAIR_DOUBLES * p;
                const int a = row >= nd ? 6 + row - nd : row - 3 * p;
                if (a >= W || (row < nd && a >= 6)) continue;
                if (is_b) v = v + o[100 + a];
                else {
                    const int cc = col >= nd ? 6 + col - nd : col - 3 * p;
                    if (cc < 0 || (col < nd && cc >= 6)) continue;
                    v = v + o[W * a + cc];
                }
            }
        }
        S[e] = v * 1000.0;
    }
}

__global__ __launch_bounds__(LVI_WAVE) void align_factor_solve(int which, const SolveHead* __restrict__ head, Work* __restrict__ wk, double* __restrict__ sys,
                                                               double* __restrict__ x_out)
{
    __shared__ double sB[am::BW * MAXND], sO[am::NB_LINEAR * MAXN], sX[MAXN];
    if (wk->reason != am::OK) return;
    const int tid = threadIdx.x, F = head->F, nd = 3 * F, nb = which == 0 ? am::NB_LINEAR : am::NB_REFINE, n = nd + nb;
    double* S = sys + (size_t)SYS_STRIDE * which;
    for (int e = tid; e < am::BW * nd; e += LVI_WAVE) sB[e] = S[e];
    for (int e = tid; e < nb * n; e += LVI_WAVE) sO[e] = S[am::off_bord(nd) + e];
    for (int e = tid; e < n; e += LVI_WAVE) sX[e] = S[am::off_b(nd, nb) + e];
    __syncthreads();
    bool ok = 2 * (nd - 3) >= n;                               // 6 (F - 1) equations for n unknowns
    double mp = DBL_MAX;
    for (int j = 0; ok && j < n; j++) {
        const double v = am::c_pivot(sB, sO, nd, n, j);        // every lane: the branch below is uniform
        if (!am::positive_finite(v)) { ok = false; break; }
        if (v < mp) mp = v;
        const int i = tid < am::BAND + nb ? am::c_row(nd, nb, j, tid) : -1;
        const double l = i >= 0 ? am::c_entry(sB, sO, nd, n, i, j, v) : 0.;
        __syncthreads();                                       // every lane has read column j's inputs
        if (i >= 0) am::c_store(sB, sO, nd, n, i, j, l);
        if (tid == 0) am::c_store(sB, sO, nd, n, j, j, v);
        __syncthreads();
    }
    if (ok) {                                                  // uniform: every lane saw the same pivots
        if (tid == 0) am::c_forward(sB, sO, nd, nb, sX);
        __syncthreads();
        for (int e = tid; e < n; e += LVI_WAVE) am::c_diag(sB, sO, nd, n, e, sX);
        __syncthreads();
        if (tid == 0) am::c_backward(sB, sO, nd, nb, sX);
    }
    if (tid == 0) {
        Work w = *wk;
        w.built = which + 1;
        if (ok) ok = am::all_finite(sX, n);
        if (!ok) {
            w.reason = am::SINGULAR; w.n_state = nd + am::NB_LINEAR; w.s = 0.; w.min_pivot[1 + which] = 0.;
            for (int k = 0; k < 3; k++) w.g_linear[k] = w.g[k] = 0.;
            for (int k = 0; k < n; k++) sX[k] = 0.;
        } else {
            w.min_pivot[1 + which] = mp;
            if (which == 0) {
                w.n_state = n;
                w.reason = am::linear_gate(sX, n, head->G, w.g_linear, &w.s, w.g0);
                for (int k = 0; k < 3; k++) w.g[k] = w.g_linear[k];
            } else {
                double lxly[6];
                am::tangent_basis(w.g0, lxly);
                am::refine_step(sX, n, lxly, head->G, w.g0);
                if (which == am::SYSTEMS - 1) {
                    sX[n - 1] = sX[n - 1] / 100.0;
                    w.n_state = n; w.s = sX[n - 1];
                    for (int k = 0; k < 3; k++) w.g[k] = w.g0[k];
                    if (w.s < 0.0) w.reason = am::NEGATIVE_SCALE_REFINED;
                }
            }
        }
        *wk = w;
    }
    __syncthreads();
    for (int e = tid; e < n; e += LVI_WAVE) S[am::off_x(nd, nb) + e] = sX[e];
    if (which == 0 || which == am::SYSTEMS - 1)                // what a solve downloads: the linear x until the last pass replaces it
        for (int e = tid; e < MAXN; e += LVI_WAVE) x_out[e] = e < n ? sX[e] : 0.;
}

struct HostFrame {
    double stamp, R[9], T[3];
    int phys, count;
    bool key, has_pre;
};

}  // namespace

struct lvi_align : Handle {
    int max_frames = 0;
    lvi_align_params P{};
    SampleStore smp;                                             // max_frames + 1 slots, as d_states
    FrameState* d_states = nullptr;
    char* d_in = nullptr; char* d_work = nullptr;                // SolveHead | FrameIn [max_frames];  Work | x [MAXN]
    double *d_pairs = nullptr, *d_sys = nullptr;
    char* h_in = nullptr; char* h_down = nullptr;                // pinned
    // the host's mirror
    std::vector<HostFrame> list;
    std::vector<int> free_slots;
    int pending = -1, pending_count = 0;                         // the slot of tmp_pre_integration, -1 before the first frame
    bool have_imu = false;
    double acc_0[3] = {}, gyr_0[3] = {};
    bool have_last = false; int last_F = 0, last_built = 0;
};

namespace {

template <class A, class B> void carve(A& a, B& pin, lvi_align* h)
{
    const size_t slots = (size_t)h->max_frames + 1;
    const size_t in_bytes = sizeof(SolveHead) + sizeof(FrameIn) * (size_t)h->max_frames;
    h->smp.carve(a, pin, slots);
    h->d_states = a.template alloc<FrameState>(slots);
    h->d_in = a.template alloc<char>(in_bytes);
    h->d_work = a.template alloc<char>(sizeof(Work) + sizeof(double) * MAXN);
    h->d_pairs = a.template alloc<double>((size_t)PAIR_DOUBLES * (MAXF - 1));
    h->d_sys = a.template alloc<double>((size_t)SYS_STRIDE * am::SYSTEMS);
    h->h_in = pin.template alloc<char>(in_bytes);
    h->h_down = pin.template alloc<char>(std::max({sizeof(FrameState) * slots, h->smp.bytes(h->smp.max_samples), sizeof(double) * (size_t)SYS_STRIDE,
                                                   sizeof(Work) + sizeof(double) * MAXN}));
}

void forget(lvi_align* h)
{
    h->list.clear();
    h->free_slots.clear();
    for (int i = h->max_frames; i >= 0; i--) h->free_slots.push_back(i);
    h->pending = -1; h->pending_count = 0; h->have_imu = false; h->have_last = false;
    for (int k = 0; k < 3; k++) h->acc_0[k] = h->gyr_0[k] = 0.;
}

void launch_job(lvi_align* h, const Job& j)
{
    hipLaunchKernelGGL(align_repropagate, dim3(1), dim3(TB), 0, h->stream, j, (const FrameIn*)nullptr, (const Work*)nullptr, h->d_states, h->smp.d_smp, h->smp.max_samples);
    LVI_HIP(hipGetLastError());
}

int find_stamp(const lvi_align* h, double stamp)
{
    for (size_t i = 0; i < h->list.size(); i++)
        if (h->list[i].stamp == stamp) return (int)i;
    return -1;
}

}  // namespace

extern "C" {

int32_t lvi_align_abi_version(void) { return LVI_ALIGN_ABI_VERSION; }

void lvi_align_params_default(lvi_align_params* p)
{
    if (!p) return;
    noise_defaults(p);
    p->TIC[0] = p->TIC[1] = p->TIC[2] = 0.;
}

int32_t lvi_align_create(int32_t device, const lvi_align_caps* caps, lvi_align** out)
{
    if (!out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!caps) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (caps->max_frames < 2 || caps->max_frames > LVI_ALIGN_MAX_FRAMES) return fail(LVI_ERR_INVALID_ARG, "max_frames is outside 2..LVI_ALIGN_MAX_FRAMES");
    if (caps->max_samples < 1 || caps->max_samples > LVI_PREINT_MAX_SAMPLES) return fail(LVI_ERR_INVALID_ARG, "max_samples is outside 1..LVI_PREINT_MAX_SAMPLES");
    return create_handle(device, out, lvi_align_destroy,
        [&](lvi_align* h) { h->max_frames = caps->max_frames; h->smp.max_samples = caps->max_samples; lvi_align_params_default(&h->P); forget(h); },
        [&](lvi_align* h) -> int32_t {
            h->open(device, [&](auto& dev, auto& pin) { carve(dev, pin, h); });
            h->smp.open();
            LVI_HIP(hipMemsetAsync(h->d_states, 0, sizeof(FrameState) * ((size_t)h->max_frames + 1), h->stream));
            LVI_HIP(hipStreamSynchronize(h->stream));
            return LVI_OK;
        });
}

void lvi_align_destroy(lvi_align* h) { destroy_with_store(h); }

int32_t lvi_align_set_params(lvi_align* h, const lvi_align_params* p)
{
    if (!h || !p) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!noise_valid(p) || !finite_n(p->TIC, 3)) return fail(LVI_ERR_INVALID_ARG, "the parameters must be finite and the noise values >= 0");
    h->P = *p;
    return LVI_OK;
}

int32_t lvi_align_clear(lvi_align* h)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    forget(h);
    return LVI_OK;
}

int32_t lvi_align_push_imu(lvi_align* h, int32_t n, const double* dt, const double* acc, const double* gyr)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (n < 0) return fail(LVI_ERR_INVALID_ARG, "n is negative");
    if (n > 0 && (!dt || !acc || !gyr)) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (n > 0 && (!finite_n(dt, (size_t)n) || !finite_n(acc, 3 * (size_t)n) || !finite_n(gyr, 3 * (size_t)n)))
        return fail(LVI_ERR_INVALID_ARG, "a sample is not finite");
    if (n == 0) return LVI_OK;
    if (h->pending >= 0 && h->pending_count + (int64_t)n > h->smp.max_samples) return fail(LVI_ERR_CAPACITY, "the pending preintegration would exceed max_samples");
    const int32_t st = h->pending < 0 ? LVI_OK : guarded(h->device, [&]() -> int32_t {
        const int at = h->pending_count;
        h->smp.stage(h->stream, h->pending, at, n, dt, acc, gyr);
        Job j{};
        j.phys = j.src = h->pending; j.src_first = j.dst_first = at; j.count = n; j.flags = J_INTEGRATE;
        launch_job(h, j);
        h->pending_count = at + n;
        return LVI_OK;
    });
    if (st != LVI_OK) return st;
    h->have_imu = true;
    for (int k = 0; k < 3; k++) { h->acc_0[k] = acc[3 * (size_t)(n - 1) + k]; h->gyr_0[k] = gyr[3 * (size_t)(n - 1) + k]; }
    return LVI_OK;
}

int32_t lvi_align_add_frame(lvi_align* h, double stamp, const double* Ba, const double* Bg)
{
    if (!h || !Ba || !Bg) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!std::isfinite(stamp) || !finite_n(Ba, 3) || !finite_n(Bg, 3)) return fail(LVI_ERR_INVALID_ARG, "the stamp and the biases must be finite");
    if (!h->list.empty() && !(stamp > h->list.back().stamp)) return fail(LVI_ERR_INVALID_ARG, "the stamp is not greater than the last frame's");
    if ((int)h->list.size() >= h->max_frames) return fail(LVI_ERR_CAPACITY, "the list holds max_frames frames");
    if (!h->have_imu) return fail(LVI_ERR_STATE, "no sample was ever pushed: acc_0 and gyr_0 are not defined");
    return guarded(h->device, [&]() -> int32_t {
        const int fresh = h->free_slots.back();                // max_frames + 1 slots for max_frames frames and the pending one
        Job j{};
        j.phys = j.src = fresh; j.flags = J_CREATE;
        for (int k = 0; k < 3; k++) { j.ba[k] = Ba[k]; j.bg[k] = Bg[k]; j.acc_0[k] = h->acc_0[k]; j.gyr_0[k] = h->gyr_0[k]; }
        launch_job(h, j);
        h->free_slots.pop_back();
        HostFrame f{};
        f.stamp = stamp; f.R[0] = f.R[4] = f.R[8] = 1.;
        f.has_pre = h->pending >= 0; f.phys = h->pending; f.count = h->pending_count;
        h->list.push_back(f);
        h->pending = fresh; h->pending_count = 0;
        return LVI_OK;
    });
}

int32_t lvi_align_erase_through(lvi_align* h, double t0)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    const int at = find_stamp(h, t0);
    if (at < 0) return fail(LVI_ERR_STATE, "t0 is no frame's stamp");
    for (int i = 0; i <= at; i++)
        if (h->list[i].has_pre) h->free_slots.push_back(h->list[i].phys);
    h->list.erase(h->list.begin(), h->list.begin() + at + 1);
    return LVI_OK;
}

int32_t lvi_align_set_pose(lvi_align* h, double stamp, const double* R, const double* T, int32_t is_key_frame)
{
    if (!h || !R || !T) return fail(LVI_ERR_INVALID_ARG, "null argument");
    const int at = find_stamp(h, stamp);
    if (at < 0) return fail(LVI_ERR_STATE, "stamp is no frame's");
    HostFrame& f = h->list[at];
    for (int k = 0; k < 9; k++) f.R[k] = R[k];
    for (int k = 0; k < 3; k++) f.T[k] = T[k];
    f.key = is_key_frame != 0;
    return LVI_OK;
}

int32_t lvi_align_frames(lvi_align* h, int32_t* count)
{
    if (!h || !count) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *count = (int32_t)h->list.size();
    return LVI_OK;
}

int32_t lvi_align_excitation(lvi_align* h, double* var)
{
    if (!h || !var) return fail(LVI_ERR_INVALID_ARG, "null argument");
    const int F = (int)h->list.size();
    if (F < 2) return fail(LVI_ERR_STATE, "fewer than two frames");
    return guarded(h->device, [&]() -> int32_t {
        download(h, h->d_states, sizeof(FrameState) * ((size_t)h->max_frames + 1));
        const FrameState* st = reinterpret_cast<const FrameState*>(h->h_down);
        std::vector<am::Pre> pre((size_t)F - 1);
        for (int i = 1; i < F; i++) copy_pre(st[h->list[i].phys].s, pre[(size_t)i - 1]);
        *var = am::excitation(pre.data(), F - 1);
        return LVI_OK;
    });
}

int32_t lvi_align_solve(lvi_align* h, double* Bgs_inout, double* g_out, double* x_out, int32_t cap, lvi_align_info* info)
{
    if (!h || !Bgs_inout || !g_out || !x_out || !info) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!finite_n(Bgs_inout, 33)) return fail(LVI_ERR_INVALID_ARG, "a bias is not finite");
    const int F = (int)h->list.size(), n4 = 3 * F + am::NB_LINEAR;
    if (cap < n4) return fail(LVI_ERR_CAPACITY, "x_out holds fewer than 3 F + 4 doubles");
    lvi_align_info r{};
    r.frames = F; r.n_state = n4;
    if (F < 2) {
        r.reason = am::TOO_FEW;
        for (int k = 0; k < n4; k++) x_out[k] = 0.;
        g_out[0] = g_out[1] = g_out[2] = 0.;
        *info = r;
        return LVI_OK;
    }
    return guarded(h->device, [&]() -> int32_t {
        SolveHead* hd = reinterpret_cast<SolveHead*>(h->h_in);
        FrameIn* fi = reinterpret_cast<FrameIn*>(h->h_in + sizeof(SolveHead));
        for (int k = 0; k < 33; k++) hd->Bgs[k] = Bgs_inout[k];
        for (int k = 0; k < 3; k++) { hd->TIC[k] = h->P.TIC[k]; hd->G[k] = h->P.G[k]; }
        hd->F = F; hd->reserved = 0;
        for (int i = 0; i < F; i++) {
            const HostFrame& f = h->list[i];
            std::memcpy(fi[i].R, f.R, sizeof(f.R));
            std::memcpy(fi[i].T, f.T, sizeof(f.T));
            fi[i].phys = f.has_pre ? f.phys : 0; fi[i].count = f.has_pre ? f.count : 0;
        }
        LVI_HIP(hipMemcpyAsync(h->d_in, h->h_in, sizeof(SolveHead) + sizeof(FrameIn) * (size_t)F, hipMemcpyHostToDevice, h->stream));
        const SolveHead* d_hd = reinterpret_cast<const SolveHead*>(h->d_in);
        const FrameIn* d_fi = reinterpret_cast<const FrameIn*>(h->d_in + sizeof(SolveHead));
        Work* d_wk = reinterpret_cast<Work*>(h->d_work);
        double* d_x = reinterpret_cast<double*>(h->d_work + sizeof(Work));
        hipLaunchKernelGGL(align_gyro, dim3(1), dim3(TB), 0, h->stream, d_hd, d_fi, h->d_states, d_wk);
        LVI_HIP(hipGetLastError());
        Job j{};
        j.flags = J_LIST;
        hipLaunchKernelGGL(align_repropagate, dim3(F - 1), dim3(TB), 0, h->stream, j, d_fi, (const Work*)d_wk, h->d_states, h->smp.d_smp, h->smp.max_samples);
        LVI_HIP(hipGetLastError());
        for (int w = 0; w < am::SYSTEMS; w++) {
            hipLaunchKernelGGL(align_system, dim3(1), dim3(TB), 0, h->stream, w, d_hd, d_fi, h->d_states, (const Work*)d_wk, h->d_pairs, h->d_sys);
            LVI_HIP(hipGetLastError());
            hipLaunchKernelGGL(align_factor_solve, dim3(1), dim3(LVI_WAVE), 0, h->stream, w, d_hd, d_wk, h->d_sys, d_x);
            LVI_HIP(hipGetLastError());
        }
        download(h, h->d_work, sizeof(Work) + sizeof(double) * (size_t)n4);
        const Work& w = *reinterpret_cast<const Work*>(h->h_down);
        const double* x = reinterpret_cast<const double*>(h->h_down + sizeof(Work));
        r.ok = w.reason == am::OK; r.reason = w.reason; r.n_state = w.n_state; r.s = w.s;
        for (int k = 0; k < 3; k++) { r.delta_bg[k] = w.delta_bg[k]; r.g_linear[k] = w.g_linear[k]; r.g[k] = w.g[k]; g_out[k] = w.g[k]; }
        for (int k = 0; k < 6; k++) r.min_pivot[k] = w.min_pivot[k];
        const bool zero = w.reason == am::SINGULAR;
        for (int k = 0; k < n4; k++) x_out[k] = (zero || k >= w.n_state) ? 0. : x[k];
        for (int k = 0; k < 33; k++) Bgs_inout[k] = w.Bgs[k];
        h->have_last = true; h->last_F = F; h->last_built = w.built;
        *info = r;
        return LVI_OK;
    });
}

int32_t lvi_align_get_frame(lvi_align* h, int32_t index, lvi_align_frame* out, int32_t cap, double* dt, double* acc, double* gyr)
{
    if (!h || !out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (index < 0 || index >= (int)h->list.size()) return fail(LVI_ERR_INVALID_ARG, "index is outside the list");
    const HostFrame& f = h->list[index];
    const int n = f.has_pre ? f.count : 0;
    if (cap < 0) return fail(LVI_ERR_INVALID_ARG, "cap is negative");
    if ((dt || acc || gyr) && cap < n) return fail(LVI_ERR_CAPACITY, "an array is shorter than the frame's samples");
    lvi_align_frame o{};
    o.stamp = f.stamp;
    std::memcpy(o.R, f.R, sizeof(o.R));
    std::memcpy(o.T, f.T, sizeof(o.T));
    o.is_key_frame = f.key; o.has_preintegration = f.has_pre; o.samples = n;
    const int32_t st = !f.has_pre ? LVI_OK : guarded(h->device, [&]() -> int32_t {
        download(h, h->d_states + f.phys, sizeof(FrameState));
        const FrameState& s = *reinterpret_cast<const FrameState*>(h->h_down);
        copy_pre(s.s, o);
        for (int k = 0; k < 3; k++) { o.linearized_acc[k] = s.linearized_acc[k]; o.linearized_gyr[k] = s.linearized_gyr[k]; }
        std::memcpy(o.jacobian, s.jacobian, sizeof(o.jacobian));
        if ((dt || acc || gyr) && n > 0) h->smp.fetch(h, f.phys, n, dt, acc, gyr);
        return LVI_OK;
    });
    if (st == LVI_OK) *out = o;
    return st;
}

int32_t lvi_align_last_system(lvi_align* h, int32_t which, int32_t* n_out, double* A, double* b, double* x, int32_t cap)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (which < 0 || which >= am::SYSTEMS) return fail(LVI_ERR_INVALID_ARG, "which is outside 0..4");
    if (!h->have_last || which >= h->last_built) return fail(LVI_ERR_STATE, "the last solve did not build this system");
    const int nd = 3 * h->last_F, nb = which == 0 ? am::NB_LINEAR : am::NB_REFINE, n = nd + nb;
    if (A && (int64_t)cap < (int64_t)n * n) return fail(LVI_ERR_CAPACITY, "A holds fewer than n * n doubles");
    if (n_out) *n_out = n;
    if (!A && !b && !x) return LVI_OK;
    return guarded(h->device, [&]() -> int32_t {
        download(h, h->d_sys + (size_t)SYS_STRIDE * which, sizeof(double) * (size_t)am::sys_doubles(nd, nb));
        const double* S = reinterpret_cast<const double*>(h->h_down);
        if (A) am::c_expand(nd, nb, S, S + am::off_bord(nd), A);
        if (b) std::memcpy(b, S + am::off_b(nd, nb), sizeof(double) * (size_t)n);
        if (x) std::memcpy(x, S + am::off_x(nd, nb), sizeof(double) * (size_t)n);
        return LVI_OK;
    });
}

int32_t lvi_align_apply(const lvi_align_params* params, int32_t frame_count, double* Ps, double* Rs, double* Vs, const double* x, int32_t n_x, double* g,
                        const double* key_R, int32_t n_key, double* rot_diff, int32_t* flags)
{
    if (!params || !Ps || !Rs || !Vs || !x || !g || (n_key > 0 && !key_R)) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (frame_count < 0 || frame_count >= LVI_PREINT_SLOTS) return fail(LVI_ERR_INVALID_ARG, "frame_count is outside 0..WINDOW_SIZE");
    if (n_key < 0 || n_x < 1 || (int64_t)n_x < 3 * (int64_t)std::min(n_key, frame_count + 1) + 1) return fail(LVI_ERR_INVALID_ARG, "x is shorter than the key frames' velocities and s");
    double rd[9];
    int fl = 0;
    am::apply(frame_count, params->TIC, Ps, Rs, Vs, x, n_x, g, key_R, n_key, rd, &fl);
    if (rot_diff) std::memcpy(rot_diff, rd, sizeof(rd));
    if (flags) *flags = fl;
    return LVI_OK;
}

}  // extern "C"
