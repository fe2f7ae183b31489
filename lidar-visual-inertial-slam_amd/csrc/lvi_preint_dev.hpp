// lvi_preint_dev.hpp — what the window's preintegration (lvi_preint.hip) and the alignment's per-image
// preintegrations (lvi_align.hip) share: the one integration body behind preint_run and align_repropagate, the
// store of a handle's samples on the host, and the small host helpers both handles use.
//
// The body.  One workgroup of 256 threads per job; a job names a slot, a run of samples, and whether the slot is created,
// repropagated with new biases or continued.  Threads 0..224 own one matrix element each (thread r * 15 + c owns (r, c));
// lanes 225..233 of the last wave build the 3 x 3 blocks of F (and V) of the NEXT step while the matrix threads multiply
// with the present one, and lane 255 runs the vector chain a chunk of samples ahead.  F and V are double buffered, so a step
// costs two barriers; a chunk of LVI_PREINT_CHUNK samples costs three more.  integrate_job<true> is the full form: jacobian
// and covariance (covariance = T F' + V noise V', the last term summed from V by the thread that owns the element and never
// stored), the navigation chain, and a run read from another slot's buffer copied behind the slot's own as it is staged.
// integrate_job<false> carries the jacobian alone: it has no covariance, no T and no V, reads no navigation state and
// integrates a run where it lies.  What one form lacks is not in its instantiation (if constexpr), nor in its kernel's LDS.
#pragma once
#include <type_traits>
#include <utility>

#include "../../include/lvi_preint.h"
#include "lvi_dev.hpp"
#include "lvi_preint_math.hpp"

namespace lvi_preint_dev {

using namespace lvi;
namespace pm = lvi_preint_math;

constexpr int TB = 256, CHUNK = LVI_PREINT_CHUNK, SD = 7;   // SD: doubles per sample: dt, acc, gyr
constexpr int NN = pm::N * pm::N;

enum { J_CREATE = 1, J_REPROP = 2, J_INTEGRATE = 4, J_NAV = 8, J_LIST = 16 };

struct Job {
    int32_t phys;                // the slot's state and the buffer the samples end in
    int32_t src, src_first;      // the buffer and the sample the run starts at
    int32_t dst_first;           // where the run lies in the slot's own buffer; the full form copies a run read elsewhere there
    int32_t count, flags;
    double ba[3], bg[3];         // J_CREATE, J_REPROP: linearized_ba / bg
    double acc_0[3], gyr_0[3];   // J_CREATE: acc_0, gyr_0
};
// what the full form reads beside its job
struct FullArgs {
    double q[pm::NV];            // the diagonal of noise
    double G[3];
    double nav_acc[3], nav_gyr[3];   // J_NAV: the estimator's acc_0, gyr_0 before the call (the host holds them)
};

// an IntegrationBase without its buffers: without its covariance, and the full record, which continues it
struct FrameState {
    pm::State s;
    double linearized_acc[3], linearized_gyr[3];
    double jacobian[NN];
};
struct SlotState : FrameState {
    double covariance[NN];
};
template <bool FULL> using Slot = std::conditional_t<FULL, SlotState, FrameState>;

// The LDS of a workgroup.  The kernel declares the arrays, each a __shared__ array of its own, and hands them over: the form
// without covariance declares no C, T or V, and the compiler sees every array start on 16 bytes (as members of one
// __shared__ struct the chain's stores of a step's geometry came out 8 bytes wide instead of 16).
template <bool FULL> struct Lds {
    double* J; double (*F)[NN]; double* S;                       // jacobian [NN], F [2][NN], the staged chunk [CHUNK * SD]
    pm::StepGeom* G;                                             // and its step geometry [CHUNK]
};
template <> struct Lds<true> : Lds<false> {
    double* C; double* T; double (*V)[pm::N * pm::NV];           // covariance [NN], T [NN], V [2][N * NV]
};

// F (and V) of step k of the chunk into the buffers of parity p
template <bool FULL> __device__ __forceinline__ void build_step(const Lds<FULL>& w, int k, int bi, int bj, int p)
{
    if constexpr (FULL) pm::build_entry(w.G[k], bi, bj, w.F[p], w.V[p]);
    else {
        double V[pm::N * pm::NV];                                  // nothing reads V here: the stores fall away and no V is built
        pm::build_entry(w.G[k], bi, bj, w.F[p], V);
    }
}

// J_LIST: the job is frame f of a list in device memory, repropagated with Ba = 0 and bg over its own samples
template <class Frame> __device__ __forceinline__ void list_job(Job& jb, const Frame& f, const double* bg)
{
    jb.phys = jb.src = f.phys; jb.src_first = jb.dst_first = 0; jb.count = f.count;
    jb.flags = J_REPROP | (f.count > 0 ? J_INTEGRATE : 0);
    for (int k = 0; k < 3; k++) { jb.ba[k] = 0.; jb.bg[k] = bg[k]; }
}

template <bool FULL>
__device__ __forceinline__ void integrate_job(const Lds<FULL>& w, const Job& jb, Slot<FULL>* slots, double* smp, int max_samples, const FullArgs* fa, pm::Nav* nav)
{
    const int tid = threadIdx.x, flags = jb.flags;
    const bool mat = tid < NN, builder = tid >= NN && tid < NN + 9, chain = tid == TB - 1;
    const int r = tid / pm::N, c = tid % pm::N, bi = (tid - NN) / 3, bj = (tid - NN) % 3;
    Slot<FULL>* st = slots + jb.phys;
    if (mat) {
        const bool fresh = flags & (J_CREATE | J_REPROP);
        w.J[tid] = fresh ? (r == c ? 1. : 0.) : st->jacobian[tid];
        if constexpr (FULL) w.C[tid] = fresh ? 0. : st->covariance[tid];
    }
    pm::State s;
    pm::Nav nv;
    double e_acc[3], e_gyr[3];
    if (chain) {
        if (flags & J_CREATE) pm::state_reset(s, jb.acc_0, jb.gyr_0, jb.ba, jb.bg);
        else if (flags & J_REPROP) pm::state_reset(s, st->linearized_acc, st->linearized_gyr, jb.ba, jb.bg);   // :40-49
        else s = st->s;
        if constexpr (FULL)
            if (flags & J_NAV) {
                nv = *nav;
                for (int k = 0; k < 3; k++) { e_acc[k] = fa->nav_acc[k]; e_gyr[k] = fa->nav_gyr[k]; }
            }
    }
    __syncthreads();
    if (flags & J_INTEGRATE) {
        const double* src = smp + ((size_t)jb.src * max_samples + jb.src_first) * SD;
        double* dst = smp + ((size_t)jb.phys * max_samples + jb.dst_first) * SD;
        int par = 0;
        for (int base = 0; base < jb.count; base += CHUNK) {
            const int m = min(CHUNK, jb.count - base);
            for (int t = tid; t < m * SD; t += TB) {
                const double v = src[(size_t)base * SD + t];
                w.S[t] = v;
                if constexpr (FULL)
                    if (src != dst) dst[(size_t)base * SD + t] = v;
            }
            __syncthreads();
            if (chain)
                for (int k = 0; k < m; k++) {
                    const double* x = w.S + SD * k;
                    pm::step_state(s, x[0], x + 1, x + 4, w.G[k]);
                    if constexpr (FULL)
                        if (flags & J_NAV) {
                            pm::nav_step(nv, e_acc, e_gyr, x[0], x + 1, x + 4, fa->G);
                            for (int a = 0; a < 3; a++) { e_acc[a] = x[1 + a]; e_gyr[a] = x[4 + a]; }
                        }
                }
            __syncthreads();
            if (builder) build_step(w, 0, bi, bj, par);
            __syncthreads();
            for (int k = 0; k < m; k++) {
                double jn = 0.;
                if (mat) {
                    jn = pm::f_dot(w.F[par], r, w.J, c);
                    if constexpr (FULL) w.T[tid] = pm::f_dot(w.F[par], r, w.C, c);
                }
                if (builder && k + 1 < m) build_step(w, k + 1, bi, bj, par ^ 1);
                __syncthreads();                                   // T is whole; nobody reads jacobian or covariance any more
                if (mat) {
                    if constexpr (FULL) w.C[tid] = pm::tf_dot(w.T, r, w.F[par], c) + pm::vqv_dot(w.V[par], fa->q, r, c);
                    w.J[tid] = jn;
                }
                __syncthreads();                                   // the step's matrices are whole; F and V of this parity are free
                par ^= 1;
            }
        }
    }
    if (mat) {
        st->jacobian[tid] = w.J[tid];
        if constexpr (FULL) st->covariance[tid] = w.C[tid];
    }
    if (chain) {
        st->s = s;
        if (flags & J_CREATE)
            for (int k = 0; k < 3; k++) { st->linearized_acc[k] = jb.acc_0[k]; st->linearized_gyr[k] = jb.gyr_0[k]; }
        if constexpr (FULL)
            if (flags & J_NAV) *nav = nv;
    }
}

// ---- the host side

// one download into the handle's pinned buffer and the call's wait
template <class H> void download(H* h, const void* d, size_t bytes)
{
    LVI_HIP(hipMemcpyAsync(h->h_down, d, bytes, hipMemcpyDeviceToHost, h->stream));
    LVI_HIP(hipStreamSynchronize(h->stream));
}

// The samples of a handle's slots on the device, max_samples x (dt, acc, gyr) a slot, and the pinned buffer one push is
// staged in.  A push does not wait for its upload: the event says when the staging buffer is free again.
struct SampleStore {
    int max_samples = 0;
    double* d_smp = nullptr;
    double* h_up = nullptr;                                      // pinned
    hipEvent_t up_done = nullptr; bool up_pending = false;       // the upload that last read h_up

    template <class A, class B> void carve(A& dev, B& pin, size_t slots)
    {
        d_smp = dev.template alloc<double>(slots * max_samples * SD);
        h_up = pin.template alloc<double>((size_t)max_samples * SD);
    }
    void open() { LVI_HIP(hipEventCreateWithFlags(&up_done, hipEventDisableTiming)); }
    void release()
    {
        if (up_done) (void)hipEventDestroy(up_done);
        up_done = nullptr;
    }
    double* slot(int phys) const { return d_smp + (size_t)phys * max_samples * SD; }
    size_t bytes(int n) const { return sizeof(double) * SD * (size_t)n; }

    // n samples behind position `at` of slot phys: enqueued, not waited for
    void stage(hipStream_t stream, int phys, int at, int n, const double* dt, const double* acc, const double* gyr)
    {
        if (up_pending) LVI_HIP(hipEventSynchronize(up_done));    // the staging buffer is free again
        for (int k = 0; k < n; k++) {
            double* o = h_up + (size_t)SD * k;
            o[0] = dt[k];
            for (int a = 0; a < 3; a++) { o[1 + a] = acc[3 * (size_t)k + a]; o[4 + a] = gyr[3 * (size_t)k + a]; }
        }
        LVI_HIP(hipMemcpyAsync(slot(phys) + (size_t)SD * at, h_up, bytes(n), hipMemcpyHostToDevice, stream));
        LVI_HIP(hipEventRecord(up_done, stream));
        up_pending = true;
    }
    // the first n samples of slot phys into those of dt [n], acc [n][3], gyr [n][3] that are given: one download and its wait
    template <class H> void fetch(H* h, int phys, int n, double* dt, double* acc, double* gyr) const
    {
        download(h, slot(phys), bytes(n));
        const double* v = reinterpret_cast<const double*>(h->h_down);
        for (int k = 0; k < n; k++) {
            if (dt) dt[k] = v[SD * k];
            for (int a = 0; a < 3; a++) {
                if (acc) acc[3 * k + a] = v[SD * k + 1 + a];
                if (gyr) gyr[3 * k + a] = v[SD * k + 4 + a];
            }
        }
    }
};

// *_destroy of a handle that embeds a SampleStore as `smp`
template <class H> void destroy_with_store(H* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->smp.release();
    h->close();
    delete h;
}

// the fields of a preintegration from the chain's state into a record that has them: lvi_win_imu, lvi_align_frame,
// lvi_imu_math::ImuPre, lvi_align_math::Pre (which has no linearized_ba / bg)
template <class T, class = void> struct has_biases : std::false_type {};
template <class T> struct has_biases<T, std::void_t<decltype(std::declval<T&>().linearized_ba)>> : std::true_type {};
template <class T> __host__ __device__ void copy_pre(const pm::State& s, T& o)
{
    o.sum_dt = s.sum_dt;
    for (int k = 0; k < 3; k++) { o.delta_p[k] = s.delta_p[k]; o.delta_v[k] = s.delta_v[k]; }
    for (int k = 0; k < 4; k++) o.delta_q[k] = s.delta_q[k];
    if constexpr (has_biases<T>::value)
        for (int k = 0; k < 3; k++) { o.linearized_ba[k] = s.linearized_ba[k]; o.linearized_bg[k] = s.linearized_bg[k]; }
}

// acc_n, gyr_n, acc_w, gyr_w, G of lvi_preint_params and lvi_align_params: the defaults and what set_params accepts
template <class P> void noise_defaults(P* p)
{
    p->acc_n = 0.08; p->gyr_n = 0.004; p->acc_w = 0.00004; p->gyr_w = 2.0e-6;
    p->G[0] = 0.; p->G[1] = 0.; p->G[2] = 9.8;
}
template <class P> bool noise_valid(const P* p)
{
    const double v[7] = {p->acc_n, p->gyr_n, p->acc_w, p->gyr_w, p->G[0], p->G[1], p->G[2]};
    return finite_n(v, 7) && p->acc_n >= 0 && p->gyr_n >= 0 && p->acc_w >= 0 && p->gyr_w >= 0;
}

}  // namespace lvi_preint_dev
