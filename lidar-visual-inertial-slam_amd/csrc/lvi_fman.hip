// lvi_fman.hip — vins_estimator's FeatureManager on the device (include/lvi_fman.h).
//
// The table is an array of lvi_fman_feature in list order.  Everything structural is ONE launch of ONE workgroup of 1024
// threads that walks the table in rounds of 1024 features with a workgroup prefix scan per round (at most four rounds):
// the id match and append of a frame, the stable compactions of the slides and of removeFailures, the feature_index of
// setDepth / getDepthVector and the record offsets of the projection emission.  A compaction reads one table and writes
// the other, so the list order survives and nothing is read after it was overwritten.  The triangulation is one lane per
// feature on a wider grid: lvi_fman_math.hpp's serial code, the same on host and device.
//
// Each structural kernel ends by counting what the host needs to size the next download (table size, getFeatureCount, the
// record counts of both emission modes), so every entry point waits once and downloads exactly what it returns.
#include <cmath>
#include <cstring>

#include "../../include/lvi_fman.h"
#include "lvi_dev.hpp"
#include "lvi_fman_math.hpp"
#include "lvi_winsys.hpp"

using namespace lvi;
using lvi_winsys::finite_all;
namespace fm = lvi_fman_math;

static_assert(sizeof(lvi_fman_obs) == 72 && sizeof(lvi_fman_feature) == 824, "lvi_fman_feature layout");
static_assert(LVI_FMAN_WINDOW == fm::WINDOW && LVI_FMAN_MAX_OBS == fm::MAX_OBS && LVI_FMAN_MAX_SWEEPS == fm::MAX_SWEEPS, "lvi_fman_math.hpp constants");
static_assert(sizeof(lvi_fman_obs) == sizeof(double) * fm::OBS_DOUBLES, "observation layout");

namespace {

constexpr int TB = 1024;                       // the one workgroup
constexpr int MAXF = LVI_FMAN_MAX_FEATURES;

enum { OP_FAILURES = 0, OP_BACK_SHIFT = 1, OP_BACK = 2, OP_FRONT = 3 };
enum { DEPTH_GET = 0, DEPTH_SET = 1, DEPTH_CLEAR = 2 };

// what every structural kernel leaves for the host (one download of 64 bytes)
struct Summary {
    int32_t status;                            // LVI_OK or the error the kernel met before it changed anything
    int32_t count, eligible, rec_window, rec_marg;
    int32_t aux;                               // corresponding: the pairs written
    lvi_fman_frame_info frame;
    lvi_fman_tri_info tri;
};
static_assert(sizeof(Summary) == 64, "Summary layout");

struct ShiftArgs { double marg_R[9], marg_P[3], new_R[9], new_P[3]; int32_t frame_count; };

// the table's counts: every thread of the workgroup calls it; tab must be visible (a barrier after the last write)
__device__ void summarize(const lvi_fman_feature* tab, int N, Summary* out, int* sh)
{
    if (threadIdx.x < 3) sh[threadIdx.x] = 0;
    __syncthreads();
    int e = 0, rw = 0, rm = 0;
    for (int i = threadIdx.x; i < N; i += TB) {
        const int k = tab[i].n_obs, s = tab[i].start_frame;
        if (fm::eligible(k, s)) { e++; rw += k - 1; if (s == 0) rm += k - 1; }
    }
    e = wave_sum(e); rw = wave_sum(rw); rm = wave_sum(rm);
    if (lane_id() == 0) { atomicAdd(&sh[0], e); atomicAdd(&sh[1], rw); atomicAdd(&sh[2], rm); }   // integers: the order does not matter
    __syncthreads();
    if (threadIdx.x == 0) { out->count = N; out->eligible = sh[0]; out->rec_window = sh[1]; out->rec_marg = sh[2]; }
}

// addFeatureCheckParallax (:45-106)
__global__ __launch_bounds__(TB) void fman_add_frame(lvi_fman_feature* tab, int N, int max_features, int frame_count, int n, const int32_t* ids,
                                                     const double* obs, double td, lvi_fman_params P, Summary* out)
{
    __shared__ int match[MAXF];                // per frame entry: the table slot (>= 0), or -2 - slot for a new feature
    __shared__ double term[MAXF];              // per feature: its parallax, -1 where it has none
    __shared__ int ws[TB / 64 + 1];
    __shared__ int sh[4];
    const int tid = threadIdx.x;
    for (int j = tid; j < n; j += TB) match[j] = -1;
    if (tid == 0) sh[3] = 0;
    __syncthreads();
    // find_if of :57-60, turned round: ids is ascending, so every table entry looks itself up (ids in the table are unique)
    for (int t = tid; t < N; t += TB) {
        const int id = tab[t].feature_id;
        int lo = 0, hi = n;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (ids[mid] < id) lo = mid + 1; else hi = mid; }
        if (lo < n && ids[lo] == id) {
            match[lo] = t;
            if (tab[t].n_obs >= LVI_FMAN_MAX_OBS || tab[t].start_frame + tab[t].n_obs > LVI_FMAN_WINDOW) sh[3] = 1;   // no room for another observation
        }
    }
    __syncthreads();
    int added = 0;
    for (int base = 0; base < n; base += TB) {
        const int j = base + tid;
        const int isnew = j < n && match[j] < 0;
        int tot;
        const int off = block_excl_scan<TB>(isnew, ws, &tot);
        if (isnew) match[j] = -2 - (N + added + off);
        added += tot;
    }
    __syncthreads();
    if (sh[3] || N + added > max_features) {                       // uniform: nothing was written yet
        if (tid == 0) out->status = sh[3] ? LVI_ERR_STATE : LVI_ERR_CAPACITY;
        return;
    }
    for (int j = tid; j < n; j += TB) {
        const double* o = obs + 8 * j;
        lvi_fman_obs ob;
        ob.point[0] = o[0]; ob.point[1] = o[1]; ob.point[2] = o[2]; ob.uv[0] = o[3]; ob.uv[1] = o[4]; ob.velocity[0] = o[5]; ob.velocity[1] = o[6];
        ob.depth = o[7]; ob.cur_td = td;
        if (match[j] >= 0) {                                       // :67-80
            lvi_fman_feature* f = tab + match[j];
            f->obs[f->n_obs] = ob;
            f->n_obs = f->n_obs + 1;
            if (ob.depth > 0 && f->lidar_depth_flag == 0) {
                f->estimated_depth = ob.depth;
                f->lidar_depth_flag = 1;
                f->obs[0].depth = ob.depth;
            }
        } else {                                                   // :62-66 and the constructor (feature_manager.h:60-74)
            lvi_fman_feature* f = tab + (-2 - match[j]);
            f->feature_id = ids[j]; f->start_frame = frame_count; f->n_obs = 1; f->solve_flag = 0; f->reserved = 0;
            if (ob.depth > 0) { f->estimated_depth = ob.depth; f->lidar_depth_flag = 1; }
            else { f->estimated_depth = -1.0; f->lidar_depth_flag = 0; }
            f->obs[0] = ob;
        }
    }
    __syncthreads();
    const int N1 = N + added, last_track_num = n - added;
    lvi_fman_frame_info fi;
    fi.last_track_num = last_track_num; fi.parallax_num = 0; fi.keyframe = 1; fi.added = added; fi.parallax_sum = 0;
    if (!(frame_count < 2 || last_track_num < 20)) {               // :83-105
        for (int i = tid; i < N1; i += TB) {
            const lvi_fman_feature* f = tab + i;
            double v = -1.0;
            if (f->start_frame <= frame_count - 2 && f->start_frame + f->n_obs - 1 >= frame_count - 1)
                v = fm::compensated_parallax2(f->obs[frame_count - 2 - f->start_frame].point, f->obs[frame_count - 1 - f->start_frame].point);
            term[i] = v;                                           // a term is max(0, .): never negative, never NaN
        }
        __syncthreads();
        if (tid == 0) {                                            // one lane, list order: the sum is the reference's bit for bit
            double sum = 0; int num = 0;
            for (int i = 0; i < N1; i++)
                if (term[i] >= 0) { sum += term[i]; num++; }
            fi.parallax_sum = sum; fi.parallax_num = num;
            fi.keyframe = num == 0 ? 1 : (sum / num >= P.min_parallax ? 1 : 0);
        }
    }
    if (tid == 0) { out->status = LVI_OK; out->frame = fi; }
    summarize(tab, N1, out, sh);
}

// removeFailures and the three slides: src -> dst, stable
__global__ __launch_bounds__(TB) void fman_compact(const lvi_fman_feature* src, lvi_fman_feature* dst, int N, int op, ShiftArgs a, lvi_fman_params P, Summary* out)
{
    __shared__ int ws[TB / 64 + 1];
    __shared__ int sh[4];
    const int tid = threadIdx.x;
    int kept = 0;
    for (int base = 0; base < N; base += TB) {
        const int i = base + tid;
        int keep = 0, erase = -1;                                  // erase: the observation that leaves
        lvi_fman_feature h;                                        // the header as it will be (obs not used)
        if (i < N) {
            const lvi_fman_feature* f = src + i;
            h.feature_id = f->feature_id; h.start_frame = f->start_frame; h.n_obs = f->n_obs; h.lidar_depth_flag = f->lidar_depth_flag;
            h.solve_flag = f->solve_flag; h.reserved = 0; h.estimated_depth = f->estimated_depth;
            keep = 1;
            if (op == OP_FAILURES) {
                keep = h.solve_flag != 2;
            } else if (op == OP_BACK_SHIFT) {                      // :285-339
                if (h.start_frame != 0) h.start_frame--;
                else {
                    double depth = -1;
                    if (f->obs[0].depth > 0) depth = f->obs[0].depth;
                    else if (h.estimated_depth > 0) depth = h.estimated_depth;
                    erase = 0; h.n_obs--;
                    if (h.n_obs < 2) keep = 0;
                    else {
                        const double dep_j = fm::shifted_depth(f->obs[0].point, depth, a.marg_R, a.marg_P, a.new_R, a.new_P);
                        if (f->obs[1].depth > 0) { h.estimated_depth = f->obs[1].depth; h.lidar_depth_flag = 1; }
                        else if (dep_j > 0) { h.estimated_depth = dep_j; h.lidar_depth_flag = 0; }
                        else { h.estimated_depth = P.init_depth; h.lidar_depth_flag = 0; }
                    }
                }
            } else if (op == OP_BACK) {                            // :341-357
                if (h.start_frame != 0) h.start_frame--;
                else { erase = 0; h.n_obs--; if (h.n_obs == 0) keep = 0; }
            } else {                                               // :359-379
                if (h.start_frame == a.frame_count) h.start_frame--;
                else {
                    const int j = LVI_FMAN_WINDOW - 1 - h.start_frame;
                    if (!(h.start_frame + h.n_obs - 1 < a.frame_count - 1) && j >= 0 && j < h.n_obs) {
                        erase = j; h.n_obs--;
                        if (h.n_obs == 0) keep = 0;
                    }
                }
            }
        }
        int tot;
        const int off = block_excl_scan<TB>(keep, ws, &tot);
        if (keep) {
            lvi_fman_feature* d = dst + kept + off;
            const lvi_fman_feature* f = src + i;
            d->feature_id = h.feature_id; d->start_frame = h.start_frame; d->n_obs = h.n_obs; d->lidar_depth_flag = h.lidar_depth_flag;
            d->solve_flag = h.solve_flag; d->reserved = 0; d->estimated_depth = h.estimated_depth;
            for (int k = 0; k < h.n_obs; k++) d->obs[k] = f->obs[(erase >= 0 && k >= erase) ? k + 1 : k];
        }
        kept += tot;
    }
    __syncthreads();
    if (tid == 0) out->status = LVI_OK;
    summarize(dst, kept, out, sh);
}

// getDepthVector / setDepth / clearDepth (:150-211): feature_index by prefix scan
__global__ __launch_bounds__(TB) void fman_depth(lvi_fman_feature* tab, int N, int what, double* x, lvi_fman_params P)
{
    __shared__ int ws[TB / 64 + 1];
    int done = 0;
    for (int base = 0; base < N; base += TB) {
        const int i = base + threadIdx.x;
        const int el = i < N && fm::eligible(tab[i].n_obs, tab[i].start_frame);
        int tot;
        const int k = done + block_excl_scan<TB>(el, ws, &tot);
        if (el) {
            lvi_fman_feature* f = tab + i;
            if (what == DEPTH_GET) x[k] = f->estimated_depth > 0 ? 1. / f->estimated_depth : 1. / P.init_depth;
            else {
                f->estimated_depth = 1.0 / x[k];
                if (what == DEPTH_SET) f->solve_flag = f->estimated_depth < 0 ? 2 : 1;
                else f->lidar_depth_flag = 0;
            }
        }
        done += tot;
    }
}

// getCorresponding (:129-148)
__global__ __launch_bounds__(TB) void fman_corresponding(const lvi_fman_feature* tab, int N, int l, int r, double* pairs, Summary* out)
{
    __shared__ int ws[TB / 64 + 1];
    int done = 0;
    for (int base = 0; base < N; base += TB) {
        const int i = base + threadIdx.x;
        const int has = i < N && tab[i].start_frame <= l && tab[i].start_frame + tab[i].n_obs - 1 >= r && l - tab[i].start_frame < tab[i].n_obs &&
                        r >= tab[i].start_frame;
        int tot;
        const int k = done + block_excl_scan<TB>(has, ws, &tot);
        if (has) {
            const lvi_fman_feature* f = tab + i;
            const double* a = f->obs[l - f->start_frame].point;
            const double* b = f->obs[r - f->start_frame].point;
            double* o = pairs + 6 * k;
            o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = b[0]; o[4] = b[1]; o[5] = b[2];
        }
        done += tot;
    }
    if (threadIdx.x == 0) out->aux = done;
}

// the factor loops of Estimator::optimization (estimator.cpp:745-789, :849-889)
__global__ __launch_bounds__(TB) void fman_projections(const lvi_fman_feature* tab, int N, int mode, lvi_fman_ids ids, lvi_marg_projection* recs, double* inv_dep,
                                                       int32_t* flags, lvi_fman_params P)
{
    __shared__ unsigned long long ws[TB / 64 + 1];
    unsigned long long done = 0;                                   // feature_index in the high word, record offset in the low
    for (int base = 0; base < N; base += TB) {
        const int i = base + threadIdx.x;
        const int el = i < N && fm::eligible(tab[i].n_obs, tab[i].start_frame);
        const int emits = el && (mode == LVI_FMAN_MODE_WINDOW || tab[i].start_frame == 0);
        const unsigned long long mine = ((unsigned long long)el << 32) | (unsigned long long)(emits ? tab[i].n_obs - 1 : 0);
        unsigned long long tot;
        const unsigned long long at = done + block_excl_scan_u64<TB>(mine, ws, &tot);
        if (el) {
            const lvi_fman_feature* f = tab + i;
            const int feature_index = (int)(at >> 32);
            inv_dep[feature_index] = f->estimated_depth > 0 ? 1. / f->estimated_depth : 1. / P.init_depth;
            flags[feature_index] = f->lidar_depth_flag;
            if (emits) {
                lvi_marg_projection* o = recs + (unsigned)(at & 0xffffffffull);
                const lvi_fman_obs& o0 = f->obs[0];
                for (int k = 1; k < f->n_obs; k++, o++) {
                    const lvi_fman_obs& oj = f->obs[k];
                    o->pose_i = ids.pose + f->start_frame; o->pose_j = ids.pose + f->start_frame + k; o->ex = ids.ex; o->feature = ids.feature + feature_index;
                    o->td = ids.td; o->reserved = 0;
                    for (int c = 0; c < 3; c++) { o->pts_i[c] = o0.point[c]; o->pts_j[c] = oj.point[c]; }
                    for (int c = 0; c < 2; c++) { o->velocity_i[c] = o0.velocity[c]; o->velocity_j[c] = oj.velocity[c]; }
                    o->td_i = o0.cur_td; o->td_j = oj.cur_td; o->row_i = o0.uv[1]; o->row_j = oj.uv[1];
                }
            }
        }
        done += tot;
    }
}

// triangulate (:213-268): one lane per feature, lvi_fman_math.hpp's serial code
__global__ __launch_bounds__(64) void fman_triangulate(lvi_fman_feature* tab, int N, fm::Poses W, lvi_fman_params P, Summary* out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= N) return;
    lvi_fman_feature* f = tab + i;
    const int k = f->n_obs, s = f->start_frame;
    if (!fm::eligible(k, s) || s < 0 || s + k > LVI_FMAN_MAX_OBS) return;
    if (f->estimated_depth > 0) return;
    int sweeps = 0;
    double depth = fm::triangulate_depth(W, s, k, &f->obs[0].point[0], &sweeps);
    atomicAdd(&out->tri.triangulated, 1);                          // integer counters: the order does not matter
    atomicMax(&out->tri.max_sweeps, sweeps);
    if (!(fabs(depth) <= 1.7976931348623157e308)) atomicAdd(&out->tri.non_finite, 1);
    if (depth < 0.0) { depth = P.init_depth; atomicAdd(&out->tri.negative, 1); }
    f->estimated_depth = depth;
}

}  // namespace

struct lvi_fman : Handle {
    int max_features = 0;
    lvi_fman_params P{};
    lvi_fman_feature* tab[2] = {nullptr, nullptr};
    int cur = 0;
    int32_t* d_ids = nullptr; double* d_obs = nullptr; double* d_x = nullptr; Summary* d_sum = nullptr;
    char* d_out = nullptr; size_t out_bytes = 0;                   // pairs, records + depths + flags
    int32_t* h_ids = nullptr; double* h_obs = nullptr; double* h_x = nullptr; Summary* h_sum = nullptr; char* h_out = nullptr;   // pinned
    Summary s{};                                                   // the table's counts after the last operation
};

namespace {

size_t rec_room(int mf) { return align256(sizeof(lvi_marg_projection) * (size_t)mf * LVI_FMAN_WINDOW); }
size_t out_room(int mf) { return std::max(rec_room(mf) + align256(8 * (size_t)mf) + align256(4 * (size_t)mf), sizeof(lvi_fman_feature) * (size_t)mf); }

template <class A, class B> void carve(A& a, B& pin, lvi_fman* h)
{
    const size_t mf = (size_t)h->max_features;
    h->out_bytes = out_room(h->max_features);
    h->tab[0] = a.template alloc<lvi_fman_feature>(mf);
    h->tab[1] = a.template alloc<lvi_fman_feature>(mf);
    alloc_pair(a, pin, h->d_ids, h->h_ids, MAXF);
    alloc_pair(a, pin, h->d_obs, h->h_obs, 8 * (size_t)MAXF);
    alloc_pair(a, pin, h->d_x, h->h_x, mf);
    alloc_pair(a, pin, h->d_sum, h->h_sum, 1);
    alloc_pair(a, pin, h->d_out, h->h_out, h->out_bytes);
}

// after the call's one wait: an error met on the device leaves the host's counts as they were
int32_t settle(lvi_fman* h, const char* what)
{
    const Summary& d = *h->h_sum;
    if (d.status != LVI_OK) return fail(d.status, what);
    h->s = d;
    return LVI_OK;
}

int32_t run_compact(lvi_fman* h, int op, const ShiftArgs& a)
{
    return guarded(h->device, [&]() -> int32_t {
        hipStream_t s = h->stream;
        LVI_HIP(hipMemsetAsync(h->d_sum, 0, sizeof(Summary), s));
        hipLaunchKernelGGL(fman_compact, dim3(1), dim3(TB), 0, s, h->tab[h->cur], h->tab[h->cur ^ 1], h->s.count, op, a, h->P, h->d_sum);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipMemcpyAsync(h->h_sum, h->d_sum, sizeof(Summary), hipMemcpyDeviceToHost, s));
        LVI_HIP(hipStreamSynchronize(s));                          // the call's one wait
        h->cur ^= 1;
        return settle(h, "compaction");
    });
}

int32_t depth_io(lvi_fman* h, int what, int32_t n, const double* x)
{
    if (!h || n < 0 || (n > 0 && !x)) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (n != h->s.eligible) return fail(LVI_ERR_INVALID_ARG, "the vector's length is not getFeatureCount()");
    if (n == 0) return LVI_OK;
    return guarded(h->device, [&]() -> int32_t {
        hipStream_t s = h->stream;
        std::memcpy(h->h_x, x, sizeof(double) * (size_t)n);
        LVI_HIP(hipMemcpyAsync(h->d_x, h->h_x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(fman_depth, dim3(1), dim3(TB), 0, s, h->tab[h->cur], h->s.count, what, h->d_x, h->P);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipStreamSynchronize(s));                          // the staging buffer is free again
        return LVI_OK;
    });
}

}  // namespace

extern "C" {

int32_t lvi_fman_abi_version(void) { return LVI_FMAN_ABI_VERSION; }

void lvi_fman_params_default(lvi_fman_params* p)
{
    if (!p) return;
    p->init_depth = 5.0; p->min_parallax = 10.0 / 460.0;
}

int32_t lvi_fman_create(int32_t device, int32_t max_features, lvi_fman** out)
{
    if (!out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (max_features < 1 || max_features > LVI_FMAN_MAX_FEATURES) return fail(LVI_ERR_INVALID_ARG, "max_features is outside 1..LVI_FMAN_MAX_FEATURES");
    return create_handle(device, out, lvi_fman_destroy,
        [&](lvi_fman* h) { h->max_features = max_features; lvi_fman_params_default(&h->P); },
        [&](lvi_fman* h) -> int32_t { h->open(device, [&](auto& dev, auto& pin) { carve(dev, pin, h); }); return LVI_OK; });
}

void lvi_fman_destroy(lvi_fman* h)
{
    if (!h) return;
    h->close();
    delete h;
}

int32_t lvi_fman_set_params(lvi_fman* h, const lvi_fman_params* p)
{
    if (!h || !p) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!std::isfinite(p->init_depth) || !(p->init_depth > 0) || !std::isfinite(p->min_parallax))
        return fail(LVI_ERR_INVALID_ARG, "init_depth must be finite and > 0, min_parallax finite");
    h->P = *p;
    return LVI_OK;
}

int32_t lvi_fman_clear(lvi_fman* h)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    h->s = Summary{};                                              // an empty table: nothing on the device is read before it is written
    return LVI_OK;
}

int32_t lvi_fman_count(lvi_fman* h, int32_t* table_size, int32_t* feature_count)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (table_size) *table_size = h->s.count;
    if (feature_count) *feature_count = h->s.eligible;
    return LVI_OK;
}

int32_t lvi_fman_add_frame(lvi_fman* h, int32_t frame_count, int32_t n, const int32_t* ids, const double* obs, double td, lvi_fman_frame_info* info_out)
{
    if (!h || n < 0 || (n > 0 && (!ids || !obs))) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (frame_count < 0 || frame_count > LVI_FMAN_WINDOW) return fail(LVI_ERR_INVALID_ARG, "frame_count is outside 0..WINDOW_SIZE");
    if (n > LVI_FMAN_MAX_FEATURES) return fail(LVI_ERR_INVALID_ARG, "more than LVI_FMAN_MAX_FEATURES observations in one frame");
    for (int k = 1; k < n; k++)
        if (!(ids[k - 1] < ids[k])) return fail(LVI_ERR_INVALID_ARG, "ids must be strictly ascending");
    return guarded(h->device, [&]() -> int32_t {
        hipStream_t s = h->stream;
        if (n > 0) {
            std::memcpy(h->h_ids, ids, sizeof(int32_t) * (size_t)n);
            std::memcpy(h->h_obs, obs, sizeof(double) * 8 * (size_t)n);
            LVI_HIP(hipMemcpyAsync(h->d_ids, h->h_ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
            LVI_HIP(hipMemcpyAsync(h->d_obs, h->h_obs, sizeof(double) * 8 * (size_t)n, hipMemcpyHostToDevice, s));
        }
        LVI_HIP(hipMemsetAsync(h->d_sum, 0, sizeof(Summary), s));
        hipLaunchKernelGGL(fman_add_frame, dim3(1), dim3(TB), 0, s, h->tab[h->cur], h->s.count, h->max_features, frame_count, n, h->d_ids, h->d_obs, td, h->P,
                           h->d_sum);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipMemcpyAsync(h->h_sum, h->d_sum, sizeof(Summary), hipMemcpyDeviceToHost, s));
        LVI_HIP(hipStreamSynchronize(s));                          // the call's one wait
        if (h->h_sum->status == LVI_ERR_CAPACITY) return fail(LVI_ERR_CAPACITY, "the frame would bring the table over max_features");
        if (h->h_sum->status == LVI_ERR_STATE) return fail(LVI_ERR_STATE, "a known feature has no room for another observation");
        const int32_t st = settle(h, "lvi_fman_add_frame");
        if (st == LVI_OK && info_out) *info_out = h->s.frame;
        return st;
    });
}

int32_t lvi_fman_triangulate(lvi_fman* h, const double* Ps, const double* Rs, const double* tic, const double* ric, lvi_fman_tri_info* info_out)
{
    if (!h || !Ps || !Rs || !tic || !ric) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!finite_all(Ps, 33) || !finite_all(Rs, 99) || !finite_all(tic, 3) || !finite_all(ric, 9)) return fail(LVI_ERR_INVALID_ARG, "a pose is not finite");
    fm::Poses W;
    std::memcpy(W.Ps, Ps, sizeof(W.Ps)); std::memcpy(W.Rs, Rs, sizeof(W.Rs)); std::memcpy(W.tic, tic, sizeof(W.tic)); std::memcpy(W.ric, ric, sizeof(W.ric));
    if (h->s.count == 0) { if (info_out) *info_out = lvi_fman_tri_info{}; return LVI_OK; }
    return guarded(h->device, [&]() -> int32_t {
        hipStream_t s = h->stream;
        LVI_HIP(hipMemsetAsync(h->d_sum, 0, sizeof(Summary), s));
        hipLaunchKernelGGL(fman_triangulate, dim3(div_up(h->s.count, 64)), dim3(64), 0, s, h->tab[h->cur], h->s.count, W, h->P, h->d_sum);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipMemcpyAsync(h->h_sum, h->d_sum, sizeof(Summary), hipMemcpyDeviceToHost, s));
        LVI_HIP(hipStreamSynchronize(s));                          // the call's one wait
        if (info_out) *info_out = h->h_sum->tri;                   // the table's structure, and with it h->s, is as it was
        return LVI_OK;
    });
}

int32_t lvi_fman_get_depth_vector(lvi_fman* h, int32_t cap, int32_t* count, double* dep)
{
    if (!h || cap < 0) return fail(LVI_ERR_INVALID_ARG, "null argument");
    const int n = h->s.eligible;
    if (dep && cap < n) return fail(LVI_ERR_CAPACITY, "the array is shorter than getFeatureCount()");
    if (count) *count = n;
    if (!dep || n == 0) return LVI_OK;
    return guarded(h->device, [&]() -> int32_t {
        hipStream_t s = h->stream;
        hipLaunchKernelGGL(fman_depth, dim3(1), dim3(TB), 0, s, h->tab[h->cur], h->s.count, (int)DEPTH_GET, h->d_x, h->P);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipMemcpyAsync(h->h_x, h->d_x, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
        LVI_HIP(hipStreamSynchronize(s));                          // the call's one wait
        std::memcpy(dep, h->h_x, sizeof(double) * (size_t)n);
        return LVI_OK;
    });
}

int32_t lvi_fman_set_depth(lvi_fman* h, int32_t n, const double* x) { return depth_io(h, DEPTH_SET, n, x); }
int32_t lvi_fman_clear_depth(lvi_fman* h, int32_t n, const double* x) { return depth_io(h, DEPTH_CLEAR, n, x); }

int32_t lvi_fman_remove_failures(lvi_fman* h)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    return run_compact(h, OP_FAILURES, ShiftArgs{});
}

int32_t lvi_fman_remove_back_shift_depth(lvi_fman* h, const double* marg_R, const double* marg_P, const double* new_R, const double* new_P)
{
    if (!h || !marg_R || !marg_P || !new_R || !new_P) return fail(LVI_ERR_INVALID_ARG, "null argument");
    ShiftArgs a{};
    std::memcpy(a.marg_R, marg_R, sizeof(a.marg_R)); std::memcpy(a.marg_P, marg_P, sizeof(a.marg_P));
    std::memcpy(a.new_R, new_R, sizeof(a.new_R)); std::memcpy(a.new_P, new_P, sizeof(a.new_P));
    return run_compact(h, OP_BACK_SHIFT, a);
}

int32_t lvi_fman_remove_back(lvi_fman* h)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    return run_compact(h, OP_BACK, ShiftArgs{});
}

int32_t lvi_fman_remove_front(lvi_fman* h, int32_t frame_count)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (frame_count < 1 || frame_count > LVI_FMAN_WINDOW) return fail(LVI_ERR_INVALID_ARG, "frame_count is outside 1..WINDOW_SIZE");
    ShiftArgs a{};
    a.frame_count = frame_count;
    return run_compact(h, OP_FRONT, a);
}

int32_t lvi_fman_corresponding(lvi_fman* h, int32_t l, int32_t r, int32_t cap, int32_t* count, double* pairs)
{
    if (!h || cap < 0) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (l < 0 || l > LVI_FMAN_WINDOW || r < 0 || r > LVI_FMAN_WINDOW) return fail(LVI_ERR_INVALID_ARG, "a frame is outside 0..WINDOW_SIZE");
    const int N = h->s.count;
    if (N == 0) { if (count) *count = 0; return LVI_OK; }
    return guarded(h->device, [&]() -> int32_t {
        hipStream_t s = h->stream;
        double* d_pairs = reinterpret_cast<double*>(h->d_out);     // 48 bytes per feature at most: within out_room
        hipLaunchKernelGGL(fman_corresponding, dim3(1), dim3(TB), 0, s, h->tab[h->cur], N, l, r, d_pairs, h->d_sum);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipMemcpyAsync(h->h_sum, h->d_sum, sizeof(Summary), hipMemcpyDeviceToHost, s));
        LVI_HIP(hipMemcpyAsync(h->h_out, d_pairs, sizeof(double) * 6 * (size_t)N, hipMemcpyDeviceToHost, s));
        LVI_HIP(hipStreamSynchronize(s));                          // the call's one wait
        const int m = h->h_sum->aux;
        if (pairs && cap < m) return fail(LVI_ERR_CAPACITY, "the array is shorter than the correspondences");
        if (count) *count = m;
        if (pairs && m > 0) std::memcpy(pairs, h->h_out, sizeof(double) * 6 * (size_t)m);
        return LVI_OK;
    });
}

int32_t lvi_fman_projections(lvi_fman* h, int32_t mode, const lvi_fman_ids* ids, int32_t cap, int32_t* count, lvi_marg_projection* records, int32_t cap_features,
                             int32_t* n_features, double* inv_dep, int32_t* lidar_flags)
{
    if (!h || !ids || cap < 0 || cap_features < 0) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (mode != LVI_FMAN_MODE_WINDOW && mode != LVI_FMAN_MODE_MARG_OLD) return fail(LVI_ERR_INVALID_ARG, "mode must be LVI_FMAN_MODE_*");
    const int R = mode == LVI_FMAN_MODE_WINDOW ? h->s.rec_window : h->s.rec_marg, E = h->s.eligible;
    if (records && cap < R) return fail(LVI_ERR_CAPACITY, "the array is shorter than the records");
    if ((inv_dep || lidar_flags) && cap_features < E) return fail(LVI_ERR_CAPACITY, "an array is shorter than getFeatureCount()");
    if (count) *count = R;
    if (n_features) *n_features = E;
    if (E == 0 || (!records && !inv_dep && !lidar_flags)) return LVI_OK;
    return guarded(h->device, [&]() -> int32_t {
        hipStream_t s = h->stream;
        // one buffer, one download: records, then the inverse depths, then the flags
        const size_t o_dep = align256(sizeof(lvi_marg_projection) * (size_t)R), o_flag = o_dep + align256(8 * (size_t)E), total = o_flag + 4 * (size_t)E;
        hipLaunchKernelGGL(fman_projections, dim3(1), dim3(TB), 0, s, h->tab[h->cur], h->s.count, mode, *ids, reinterpret_cast<lvi_marg_projection*>(h->d_out),
                           reinterpret_cast<double*>(h->d_out + o_dep), reinterpret_cast<int32_t*>(h->d_out + o_flag), h->P);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipMemcpyAsync(h->h_out, h->d_out, total, hipMemcpyDeviceToHost, s));
        LVI_HIP(hipStreamSynchronize(s));                          // the call's one wait
        if (records && R > 0) std::memcpy(records, h->h_out, sizeof(lvi_marg_projection) * (size_t)R);
        if (inv_dep) std::memcpy(inv_dep, h->h_out + o_dep, 8 * (size_t)E);
        if (lidar_flags) std::memcpy(lidar_flags, h->h_out + o_flag, 4 * (size_t)E);
        return LVI_OK;
    });
}

int32_t lvi_fman_download(lvi_fman* h, int32_t cap, int32_t* count, lvi_fman_feature* features)
{
    if (!h || cap < 0) return fail(LVI_ERR_INVALID_ARG, "null argument");
    const int N = h->s.count;
    if (features && cap < N) return fail(LVI_ERR_CAPACITY, "the array is shorter than the table");
    if (count) *count = N;
    if (!features || N == 0) return LVI_OK;
    return guarded(h->device, [&]() -> int32_t {
        const size_t bytes = sizeof(lvi_fman_feature) * (size_t)N;
        LVI_HIP(hipMemcpyAsync(h->h_out, h->tab[h->cur], bytes, hipMemcpyDeviceToHost, h->stream));
        LVI_HIP(hipStreamSynchronize(h->stream));                  // the call's one wait
        std::memcpy(features, h->h_out, bytes);
        return LVI_OK;
    });
}

}  // extern "C"
