// lvi_preint.hip — the IMU preintegration of vins_estimator's sliding window on the device (include/lvi_preint.h).
//
// One kernel, preint_run: the full form of the integration body of lvi_preint_dev.hpp, which describes it.  A launch runs a
// list of at most LVI_PREINT_SLOTS jobs, one workgroup of 256 threads per job.  LDS per workgroup: jacobian, covariance and
// T (3 x 1800 B), two F (2 x 1800 B), two V (2 x 2160 B), LVI_PREINT_CHUNK samples (896 B) and their step geometry
// (3584 B): 17.4 KB.
//
// What follows from the caller's own arguments lives on the host: which slots exist, how many samples each holds, the biases
// of the navigation state, and the estimator's acc_0 / gyr_0 / first_imu (the last sample pushed), which a launch receives as
// arguments.  So no entry point waits in order to validate, and the device holds only what the kernel computes.
#include <cmath>
#include <cstring>

#include "lvi_preint_dev.hpp"

using namespace lvi_preint_dev;

static_assert(sizeof(lvi_win_imu) == 16 + 8 * (1 + 3 + 4 + 3 + 3 + 3 + 225 + 225), "lvi_win_imu layout");
static_assert(sizeof(lvi_preint_nav) == sizeof(pm::Nav) && sizeof(lvi_preint_nav) == 8 * 21, "lvi_preint_nav layout");
static_assert(sizeof(pm::StepGeom) == 8 * 28 && sizeof(pm::State) == 8 * 23, "lvi_preint_math.hpp layouts");

namespace {

constexpr int SLOTS = LVI_PREINT_SLOTS;

struct Launch {
    Job job[SLOTS];
    FullArgs x;
    int32_t max_samples, reserved;
};
static_assert(sizeof(Launch) < 4096, "the launch description travels as a kernel argument");

__global__ __launch_bounds__(TB) void preint_run(Launch L, SlotState* slots, double* smp, pm::Nav* nav)
{
    __shared__ double sJ[NN], sF[2][NN], sS[CHUNK * SD], sC[NN], sT[NN], sV[2][pm::N * pm::NV];
    __shared__ pm::StepGeom sG[CHUNK];
    integrate_job<true>({{sJ, sF, sS, sG}, sC, sT, sV}, L.job[blockIdx.x], slots, smp, L.max_samples, &L.x, nav);
}

}  // namespace

struct lvi_preint : Handle {
    lvi_preint_params P{};
    SampleStore smp;                                            // SLOTS slots
    SlotState* d_slots = nullptr; pm::Nav* d_nav = nullptr;
    char* h_down = nullptr; pm::Nav* h_nav = nullptr;           // pinned
    // the host's mirror: what a call is checked against
    int map[SLOTS] = {};                                        // window slot -> the physical slot that holds it
    int count[SLOTS] = {}; bool created[SLOTS] = {};            // by physical slot
    bool first_imu = false;
    double acc_0[3] = {}, gyr_0[3] = {}, nav_Ba[3] = {}, nav_Bg[3] = {};
};

namespace {

template <class A, class B> void carve(A& a, B& pin, lvi_preint* h)
{
    h->smp.carve(a, pin, SLOTS);
    h->d_slots = a.template alloc<SlotState>(SLOTS);
    h->d_nav = a.template alloc<pm::Nav>(1);
    h->h_down = pin.template alloc<char>(std::max(sizeof(SlotState), h->smp.bytes(h->smp.max_samples)));
    h->h_nav = pin.template alloc<pm::Nav>(1);
}

void fill_launch(const lvi_preint* h, Launch& L)
{
    std::memset(&L, 0, sizeof(L));
    pm::noise_diag(h->P.acc_n, h->P.gyr_n, h->P.acc_w, h->P.gyr_w, L.x.q);
    for (int k = 0; k < 3; k++) L.x.G[k] = h->P.G[k];
    L.max_samples = h->smp.max_samples;
}

void launch(lvi_preint* h, const Launch& L, int jobs)
{
    hipLaunchKernelGGL(preint_run, dim3(jobs), dim3(TB), 0, h->stream, L, h->d_slots, h->smp.d_smp, h->d_nav);
    LVI_HIP(hipGetLastError());
}

// a fresh IntegrationBase{acc_0, gyr_0, nav.Ba, nav.Bg} in physical slot `phys`
Job fresh_job(const lvi_preint* h, int phys)
{
    Job j{};
    j.phys = j.src = phys; j.flags = J_CREATE;
    for (int k = 0; k < 3; k++) { j.ba[k] = h->nav_Ba[k]; j.bg[k] = h->nav_Bg[k]; j.acc_0[k] = h->acc_0[k]; j.gyr_0[k] = h->gyr_0[k]; }
    return j;
}

int32_t upload_nav(lvi_preint* h, const pm::Nav& n)
{
    return guarded(h->device, [&]() -> int32_t {
        LVI_HIP(hipStreamSynchronize(h->stream));                  // the staging word is free, and what was enqueued saw the old state
        *h->h_nav = n;
        LVI_HIP(hipMemcpyAsync(h->d_nav, h->h_nav, sizeof(pm::Nav), hipMemcpyHostToDevice, h->stream));
        LVI_HIP(hipStreamSynchronize(h->stream));
        for (int k = 0; k < 3; k++) { h->nav_Ba[k] = n.Ba[k]; h->nav_Bg[k] = n.Bg[k]; }
        return LVI_OK;
    });
}

void forget(lvi_preint* h)
{
    for (int i = 0; i < SLOTS; i++) { h->map[i] = i; h->count[i] = 0; h->created[i] = false; }
    h->first_imu = false;
    for (int k = 0; k < 3; k++) h->acc_0[k] = h->gyr_0[k] = 0.;
}

pm::Nav nav_identity()
{
    pm::Nav n{};
    n.R[0] = n.R[4] = n.R[8] = 1.;
    return n;
}

int32_t slot_of(lvi_preint* h, int32_t slot, int* phys)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (slot < 0 || slot >= SLOTS) return fail(LVI_ERR_INVALID_ARG, "slot is outside 0..WINDOW_SIZE");
    if (!h->created[h->map[slot]]) return fail(LVI_ERR_STATE, "the slot does not exist");
    *phys = h->map[slot];
    return LVI_OK;
}

void to_record(const SlotState& st, lvi_win_imu* o)
{
    o->pose_i = o->speed_bias_i = o->pose_j = o->speed_bias_j = 0;
    copy_pre(st.s, *o);
    std::memcpy(o->jacobian, st.jacobian, sizeof(o->jacobian));
    std::memcpy(o->covariance, st.covariance, sizeof(o->covariance));
}

}  // namespace

extern "C" {

int32_t lvi_preint_abi_version(void) { return LVI_PREINT_ABI_VERSION; }

void lvi_preint_params_default(lvi_preint_params* p)
{
    if (p) noise_defaults(p);
}

int32_t lvi_preint_create(int32_t device, const lvi_preint_caps* caps, lvi_preint** out)
{
    if (!out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!caps) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (caps->max_samples < 1 || caps->max_samples > LVI_PREINT_MAX_SAMPLES) return fail(LVI_ERR_INVALID_ARG, "max_samples is outside 1..LVI_PREINT_MAX_SAMPLES");
    return create_handle(device, out, lvi_preint_destroy,
        [&](lvi_preint* h) { h->smp.max_samples = caps->max_samples; lvi_preint_params_default(&h->P); forget(h); },
        [&](lvi_preint* h) -> int32_t {
            h->open(device, [&](auto& dev, auto& pin) { carve(dev, pin, h); });
            h->smp.open();
            LVI_HIP(hipMemsetAsync(h->d_slots, 0, sizeof(SlotState) * SLOTS, h->stream));
            return upload_nav(h, nav_identity());
        });
}

void lvi_preint_destroy(lvi_preint* h) { destroy_with_store(h); }

int32_t lvi_preint_set_params(lvi_preint* h, const lvi_preint_params* p)
{
    if (!h || !p) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!noise_valid(p)) return fail(LVI_ERR_INVALID_ARG, "the parameters must be finite and the noise values >= 0");
    h->P = *p;
    return LVI_OK;
}

int32_t lvi_preint_clear(lvi_preint* h)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    const int32_t st = upload_nav(h, nav_identity());
    if (st != LVI_OK) return st;
    forget(h);
    return LVI_OK;
}

int32_t lvi_preint_set_nav(lvi_preint* h, const lvi_preint_nav* nav)
{
    if (!h || !nav) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!finite_n(nav->P, 21)) return fail(LVI_ERR_INVALID_ARG, "the navigation state is not finite");
    pm::Nav n;
    std::memcpy(&n, nav, sizeof(n));
    return upload_nav(h, n);
}

int32_t lvi_preint_get_nav(lvi_preint* h, lvi_preint_nav* nav)
{
    if (!h || !nav) return fail(LVI_ERR_INVALID_ARG, "null argument");
    return guarded(h->device, [&]() -> int32_t {
        download(h, h->d_nav, sizeof(pm::Nav));
        std::memcpy(nav, h->h_down, sizeof(pm::Nav));
        return LVI_OK;
    });
}

int32_t lvi_preint_push(lvi_preint* h, int32_t frame_count, int32_t n, const double* dt, const double* acc, const double* gyr)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (frame_count < 0 || frame_count >= SLOTS) return fail(LVI_ERR_INVALID_ARG, "frame_count is outside 0..WINDOW_SIZE");
    if (n < 0) return fail(LVI_ERR_INVALID_ARG, "n is negative");
    if (n > 0 && (!dt || !acc || !gyr)) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (n > 0 && (!finite_n(dt, (size_t)n) || !finite_n(acc, 3 * (size_t)n) || !finite_n(gyr, 3 * (size_t)n)))
        return fail(LVI_ERR_INVALID_ARG, "a sample is not finite");
    if (n == 0) return LVI_OK;
    const int phys = h->map[frame_count];
    const bool integrate = frame_count != 0;
    if (integrate && (h->created[phys] ? h->count[phys] : 0) + (int64_t)n > h->smp.max_samples)
        return fail(LVI_ERR_CAPACITY, "the slot would exceed max_samples");
    return guarded(h->device, [&]() -> int32_t {
        Launch L;
        fill_launch(h, L);
        double a0[3], g0[3];                                       // the estimator's acc_0, gyr_0 as the slot's constructor sees them (:84-94)
        for (int k = 0; k < 3; k++) { a0[k] = h->first_imu ? h->acc_0[k] : acc[k]; g0[k] = h->first_imu ? h->gyr_0[k] : gyr[k]; }
        Job& j = L.job[0];
        j.phys = j.src = phys; j.flags = 0;
        const int at = h->created[phys] ? h->count[phys] : 0;
        if (!h->created[phys]) {
            j.flags |= J_CREATE;
            for (int k = 0; k < 3; k++) { j.ba[k] = h->nav_Ba[k]; j.bg[k] = h->nav_Bg[k]; j.acc_0[k] = a0[k]; j.gyr_0[k] = g0[k]; }
        }
        for (int k = 0; k < 3; k++) { L.x.nav_acc[k] = a0[k]; L.x.nav_gyr[k] = g0[k]; }
        if (integrate) {
            j.flags |= J_INTEGRATE | J_NAV;
            j.src_first = j.dst_first = at; j.count = n;
            h->smp.stage(h->stream, phys, at, n, dt, acc, gyr);
        }
        if (j.flags) launch(h, L, 1);                              // frame_count == 0 on a slot that exists: only acc_0 and gyr_0 move
        h->created[phys] = true;
        if (integrate) h->count[phys] = at + n;
        h->first_imu = true;
        for (int k = 0; k < 3; k++) { h->acc_0[k] = acc[3 * (size_t)(n - 1) + k]; h->gyr_0[k] = gyr[3 * (size_t)(n - 1) + k]; }
        return LVI_OK;
    });
}

int32_t lvi_preint_repropagate(lvi_preint* h, uint32_t mask, const double* Bas, const double* Bgs)
{
    if (!h || !Bas || !Bgs) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (mask >> SLOTS) return fail(LVI_ERR_INVALID_ARG, "the mask names a slot outside 0..WINDOW_SIZE");
    if (!finite_n(Bas, 3 * SLOTS) || !finite_n(Bgs, 3 * SLOTS)) return fail(LVI_ERR_INVALID_ARG, "a bias is not finite");
    for (int i = 0; i < SLOTS; i++)
        if (((mask >> i) & 1u) && !h->created[h->map[i]]) return fail(LVI_ERR_STATE, "a slot in the mask does not exist");
    if (mask == 0) return LVI_OK;
    return guarded(h->device, [&]() -> int32_t {
        Launch L;
        fill_launch(h, L);
        int jobs = 0;
        for (int i = 0; i < SLOTS; i++) {
            if (!((mask >> i) & 1u)) continue;
            Job& j = L.job[jobs++];
            j.phys = j.src = h->map[i]; j.count = h->count[h->map[i]];
            j.flags = J_REPROP | (j.count > 0 ? J_INTEGRATE : 0);
            for (int k = 0; k < 3; k++) { j.ba[k] = Bas[3 * i + k]; j.bg[k] = Bgs[3 * i + k]; }
        }
        launch(h, L, jobs);
        return LVI_OK;
    });
}

int32_t lvi_preint_slide_old(lvi_preint* h)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!h->first_imu) return fail(LVI_ERR_STATE, "no sample was ever pushed: acc_0 and gyr_0 are not defined");
    return guarded(h->device, [&]() -> int32_t {
        const int freed = h->map[0];
        Launch L;
        fill_launch(h, L);
        L.job[0] = fresh_job(h, freed);
        launch(h, L, 1);
        for (int i = 0; i + 1 < SLOTS; i++) h->map[i] = h->map[i + 1];
        h->map[SLOTS - 1] = freed;
        h->created[freed] = true; h->count[freed] = 0;
        return LVI_OK;
    });
}

int32_t lvi_preint_slide_new(lvi_preint* h)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    const int p9 = h->map[SLOTS - 2], p10 = h->map[SLOTS - 1];
    if (!h->created[p9] || !h->created[p10]) return fail(LVI_ERR_STATE, "slots 9 and 10 must exist");
    if (h->count[p9] + h->count[p10] > h->smp.max_samples) return fail(LVI_ERR_CAPACITY, "slot 9 has too little room for slot 10's samples");
    return guarded(h->device, [&]() -> int32_t {
        Launch L;
        fill_launch(h, L);
        int jobs = 0;
        if (h->count[p10] > 0) {
            Job& j = L.job[jobs++];
            j.phys = p9; j.src = p10; j.src_first = 0; j.dst_first = h->count[p9]; j.count = h->count[p10]; j.flags = J_INTEGRATE;
        }
        L.job[jobs++] = fresh_job(h, p10);                         // its state only: the other job reads slot 10's samples, not its state
        launch(h, L, jobs);
        h->count[p9] += h->count[p10];
        h->count[p10] = 0;
        return LVI_OK;
    });
}

int32_t lvi_preint_get(lvi_preint* h, int32_t slot, lvi_win_imu* out, int32_t* samples)
{
    int phys = 0;
    if (const int32_t bad = slot_of(h, slot, &phys)) return bad;
    const int32_t st = !out ? LVI_OK : guarded(h->device, [&]() -> int32_t {
        download(h, h->d_slots + phys, sizeof(SlotState));
        to_record(*reinterpret_cast<const SlotState*>(h->h_down), out);
        return LVI_OK;
    });
    if (st == LVI_OK && samples) *samples = h->count[phys];        // an error leaves both outputs as they were
    return st;
}

int32_t lvi_preint_get_samples(lvi_preint* h, int32_t slot, int32_t cap, int32_t* count, double* dt, double* acc, double* gyr)
{
    int phys = 0;
    if (const int32_t bad = slot_of(h, slot, &phys)) return bad;
    if (cap < 0) return fail(LVI_ERR_INVALID_ARG, "cap is negative");
    const int n = h->count[phys];
    if ((dt || acc || gyr) && cap < n) return fail(LVI_ERR_CAPACITY, "an array is shorter than the slot's samples");
    if (count) *count = n;
    if ((!dt && !acc && !gyr) || n == 0) return LVI_OK;
    return guarded(h->device, [&]() -> int32_t {
        h->smp.fetch(h, phys, n, dt, acc, gyr);
        return LVI_OK;
    });
}

int32_t lvi_preint_evaluate(lvi_preint* h, int32_t slot, const double* pose_i, const double* sb_i, const double* pose_j, const double* sb_j, double* residual,
                            double* jacobians)
{
    int phys = 0;
    if (const int32_t bad = slot_of(h, slot, &phys)) return bad;
    if (!pose_i || !sb_i || !pose_j || !sb_j || !residual) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!finite_n(pose_i, 7) || !finite_n(sb_i, 9) || !finite_n(pose_j, 7) || !finite_n(sb_j, 9)) return fail(LVI_ERR_INVALID_ARG, "a block is not finite");
    return guarded(h->device, [&]() -> int32_t {
        namespace im = lvi_imu_math;
        download(h, h->d_slots + phys, sizeof(SlotState));
        const SlotState& st = *reinterpret_cast<const SlotState*>(h->h_down);
        std::vector<double> buf(225 * 4 + 15 + 15 * 30);
        double *S = buf.data(), *work = S + 225, *r = work + 675, *J = r + 15;
        if (!im::imu_sqrt_info(st.covariance, S, work)) return fail(LVI_ERR_STATE, "the slot's covariance is not positive definite");
        im::ImuPre p;
        copy_pre(st.s, p);
        std::memcpy(p.jacobian, st.jacobian, sizeof(p.jacobian));
        im::imu_eval_raw(pose_i, sb_i, pose_j, sb_j, p, h->P.G, r, jacobians ? J : nullptr);
        for (int i = 0; i < 15; i++) residual[i] = im::imu_info_dot(S, i, r, 1, 0);
        if (jacobians) {
            const int col0[4] = {im::C_POSE_I, im::C_SB_I, im::C_POSE_J, im::C_SB_J}, local[4] = {6, 9, 6, 9}, size[4] = {7, 9, 7, 9};
            double* o = jacobians;
            for (int b = 0; b < 4; b++) {
                for (int i = 0; i < 15; i++)
                    for (int cc = 0; cc < size[b]; cc++) o[size[b] * i + cc] = cc < local[b] ? im::imu_info_dot(S, i, J, im::IMU_COLS, col0[b] + cc) : 0.;
                o += 15 * size[b];
            }
        }
        return LVI_OK;
    });
}

}  // extern "C"
