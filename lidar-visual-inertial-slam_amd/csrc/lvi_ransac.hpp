// What the RANSAC of rejectWithF (lvi_fmat.hip) and the RANSAC of findConnection (lvi_pnp.hip)
// stand on: OpenCV's RANSACPointSetRegistrator (ptsetreg.cpp) restated once.
//
//   host     cv::RNG((uint64)-1), getSubset's draw and attempt loop, the sample stream of one call, and
//            RANSACUpdateNumIters as a table of log(1 - (1 - ep)^M) per inlier count, so the device walk never calls log
//            or pow; then the 7-point callback's checkSubset and findFundamentalMat's stream.  No HIP in this part: tests
//            compile it with a stand-alone main under the host sanitizers.
//   device   the sequential walk of RANSACPointSetRegistrator::run over per-candidate inlier counts, and the status sweep
//   Io       the handle core (lvi_dev.hpp) and the buffer pairs of a handle (Bufs), the last call's sample stream (Trace), and the tail of a
//            call: upload, launches, download, wait.  The batched RANSAC (lvi_fmatb) takes Bufs and one Trace
//            per slot and has a tail of its own.
//
// The draws do not depend on any model, so the whole stream is known before the first hypothesis is scored.  The host
// functions are static: with external linkage the position-independent library calls them through the PLT, and
// have_collinear runs twice per subset.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

namespace lvi_ransac {

// ---------------------------------------------------------------------------------------------- host: the sample stream
// cv::RNG: multiply-with-carry, state seeded with (uint64)-1; uniform(a, b) = a == b ? a : next() % (b - a) + a
struct CvRng {
    uint64_t s = ~(uint64_t)0;
    uint32_t next() { s = (uint64_t)(uint32_t)s * 4164903690u + (uint32_t)(s >> 32); return (uint32_t)s; }
    int uniform(int a, int b) { return a == b ? a : (int)(next() % (uint32_t)(b - a) + (uint32_t)a); }
};

// getSubset: M distinct indices in [0, n), a duplicate is redrawn (n >= M or the redraw never ends), then checkSubset;
// false after max_attempts rejected subsets
template <int M, class Check>
static inline bool get_subset(CvRng& rng, int n, int max_attempts, Check&& check_subset, int32_t* idx)
{
    for (int it = 0; it < max_attempts; ++it) {
        for (int i = 0; i < M; ++i) {
            auto drawn = [&](int k) { for (int j = 0; j < i; ++j) if (idx[j] == k) return true; return false; };
            int k = rng.uniform(0, n);
            while (drawn(k)) k = rng.uniform(0, n);
            idx[i] = k;
        }
        if (check_subset(idx)) return true;
    }
    return false;
}

// subsets [count][M]: the stream of one call, which ends where getSubset first fails.  Returns the subsets before
// that; 0 when n < M.
template <int M, class Check>
static inline int sample_stream(int n, int count, int max_attempts, Check&& check_subset, int32_t* subsets)
{
    if (n < M) return 0;
    CvRng rng;
    int nsub = 0;
    while (nsub < count && get_subset<M>(rng, n, max_attempts, check_subset, subsets + M * nsub)) nsub++;
    return nsub;
}

// An entry of the table logtab [n + 1] the device walk reads: log(1 - (1 - ep)^M) for ep = (n - good) / n, from the host
// C library; +inf marks denom < DBL_MIN (RANSACUpdateNumIters returns 0 there)
template <int M>
static inline double update_log(int n, int good)
{
    double ep = (double)(n - good) / n;
    ep = std::max(ep, 0.); ep = std::min(ep, 1.);
    const double denom = 1. - std::pow(1. - ep, M);
    if (denom < DBL_MIN) return HUGE_VAL;
    return std::log(denom);
}

// log(max(1 - p, DBL_MIN)), the numerator of RANSACUpdateNumIters
static inline double num_log(double confidence) { return std::log(std::max(1. - std::min(std::max(confidence, 0.), 1.), DBL_MIN)); }

// RANSACUpdateNumIters(p, ep, M, max_iters) in its host form, for LMeDS's fixed count
template <int M>
static inline int update_num_iters(double p, double ep, int max_iters)
{
    ep = std::max(ep, 0.); ep = std::min(ep, 1.);
    const double num = num_log(p);
    double denom = 1. - std::pow(1. - ep, M);
    if (denom < DBL_MIN) return 0;
    denom = std::log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)std::lrint(num / denom);
}

// ---------------------------------------------------------------------------------------------- host: the 7-point callback
constexpr int FM_MODEL_POINTS = 7;
constexpr int FM_RANSAC_MAX_ATTEMPTS = 10000;   // RANSACPointSetRegistrator::run: getSubset(..., rng, 10000)
constexpr int FM_LMEDS_MAX_ATTEMPTS = 1000;     // LMeDSPointSetRegistrator::run: getSubset's default maxAttempts
constexpr double FM_LMEDS_OUTLIER_RATIO = 0.45;

// haveCollinearPoints (fundam.cpp) over xy [n][4] = (x1, y1, x2, y2), stride_off 0 or 2 choosing the point set: the last
// point of the subset against every pair of earlier ones, float differences
static inline bool have_collinear(const float* xy, const int32_t* idx, int stride_off)
{
    const int i = FM_MODEL_POINTS - 1;
    auto X = [&](int k) { return xy[4 * idx[k] + stride_off]; };
    auto Y = [&](int k) { return xy[4 * idx[k] + stride_off + 1]; };
    for (int j = 0; j < i; j++) {
        const double dx1 = X(j) - X(i), dy1 = Y(j) - Y(i);
        for (int k = 0; k < j; k++) {
            const double dx2 = X(k) - X(i), dy2 = Y(k) - Y(i);
            if (std::fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (std::fabs(dx1) + std::fabs(dy1) + std::fabs(dx2) + std::fabs(dy2))) return true;
        }
    }
    return false;
}

// FMEstimatorCallback::checkSubset: neither point set of the subset is degenerate; check = 0 switches it off
static inline bool fm_check_subset(const float* xy, const int32_t* idx, int check) { return !check || (!have_collinear(xy, idx, 0) && !have_collinear(xy, idx, 2)); }

// findFundamentalMat's stream on n > 7 points: max_iters subsets for RANSAC, LMeDS's fixed count (at least 3) otherwise,
// either clamped to the max_iters the handle has room for.  *niters0 is the count asked for.
static inline int fm_sample_stream(const float* xy, int n, bool ransac, int max_iters, double confidence, int check, int32_t* subsets, int* niters0)
{
    *niters0 = ransac ? std::max(max_iters, 1) : std::max(update_num_iters<FM_MODEL_POINTS>(confidence, FM_LMEDS_OUTLIER_RATIO, max_iters), 3);
    *niters0 = std::min(*niters0, max_iters);                  // LMeDS's floor of 3 can exceed a tiny max_iters
    return sample_stream<FM_MODEL_POINTS>(n, *niters0, ransac ? FM_RANSAC_MAX_ATTEMPTS : FM_LMEDS_MAX_ATTEMPTS,
                                          [&](const int32_t* idx) { return fm_check_subset(xy, idx, check); }, subsets);
}

}  // namespace lvi_ransac

#ifdef __HIPCC__
#include "lvi_dev.hpp"

namespace lvi_ransac {

// ---------------------------------------------------------------------------------------------- device
// RANSACUpdateNumIters(p, ep, M, max_iters) from the precomputed log(denom)
__device__ __forceinline__ int update_iters(double num, double ld, int max_iters)
{
    if (ld == HUGE_VAL) return 0;
    return ld >= 0 || -num >= max_iters * (-ld) ? max_iters : (int)rint(num / ld);
}

struct Walk { int iter, best_iter, best_root; };

// RANSACPointSetRegistrator::run replayed by one lane: hypothesis iter has nmodels[iter] candidates whose inlier counts
// are score[stride * iter + m].  A hypothesis without a model is skipped, but it counts as an iteration.
template <int M>
__device__ __forceinline__ Walk ransac_walk(const int* nmodels, const int* score, int stride, int nsub, int niters0, double num, const double* logtab)
{
    Walk w{0, -1, -1};
    int max_good = 0;
    for (int niters = niters0; w.iter < niters; w.iter++) {
        if (w.iter >= nsub) break;                             // getSubset failed (iter > 0 here, or nsub == 0)
        const int nm = nmodels[w.iter];
        for (int m = 0; m < nm; m++) {
            const int good = score[stride * w.iter + m];
            if (good > max(max_good, M - 1)) {
                w.best_iter = w.iter; w.best_root = m; max_good = good;
                niters = update_iters(num, logtab[good], niters);
            }
        }
    }
    return w;
}

// status[i] = inlier(i) over the wave, 64 points per round; every lane returns the number of inliers
template <class Inlier>
__device__ __forceinline__ int status_sweep(int n, unsigned char* status, Inlier&& inlier)
{
    const int lane = threadIdx.x;
    int good = 0;
    for (int base = 0; base < n; base += LVI_WAVE) {
        const int i = base + lane;
        bool in = false;
        if (i < n) {
            in = inlier(i);
            status[i] = in ? 1 : 0;
        }
        good += __popcll(__ballot(in));
    }
    return good;
}

// ---------------------------------------------------------------------------------------------- the handle's plumbing
// the handle core and the buffer pairs; a batched handle (lvi_fmatb) lays one region per slot into each block
struct Bufs : lvi::Handle {
    char* d_in = nullptr;                  // points | subsets | logtab, laid out by the owner
    char* h_in = nullptr;                  // pinned mirror of d_in
    char* d_out = nullptr;                 // info | status
    char* h_out = nullptr;

    // under the guard of create: the buffer pairs, then hyp(dev) carves the owner's per-hypothesis arrays
    template <class Hyp> void open(int dev, size_t in_bytes, size_t out_bytes, Hyp&& hyp)
    {
        lvi::Handle::open(dev, [&](auto& a, auto& pin) {
            lvi::alloc_pair(a, pin, d_in, h_in, in_bytes);
            lvi::alloc_pair(a, pin, d_out, h_out, out_bytes);
            hyp(a);
        });
    }
};

// the sample stream of the last call, kept on the host for the trace; a batched handle has one per slot
struct Trace {
    int last_nsub = 0;
    std::vector<int32_t> last_subsets;

    void record(const int32_t* sub, int model_points, int nsub)
    {
        last_nsub = nsub;
        last_subsets.assign(sub, sub + model_points * (size_t)nsub);
    }
    void clear() { last_nsub = 0; last_subsets.clear(); }

    // the head of a trace: the last call's subset count to *n_out, its first min(cap, count) subsets copied; returns that minimum
    int trace_subsets(int32_t* subsets, int model_points, int cap, int32_t* n_out) const
    {
        const int m = std::min(cap, last_nsub);
        if (n_out) *n_out = last_nsub;
        if (m > 0 && subsets) std::memcpy(subsets, last_subsets.data(), sizeof(int32_t) * model_points * (size_t)m);
        return m;
    }
};

// a handle of one point set per call: the buffers, the trace and the tail of a call
struct Io : Bufs, Trace {
    // The tail of a call.  One upload of the first `up` bytes of h_in, then launch(d_info, d_status) enqueues the
    // kernels, then one download of the info record and n status bytes, and one wait.
    template <class Info, class Launch>
    void run(size_t up, int n, double stream_us, uint8_t* status_out, Info* info_out, Launch&& launch)
    {
        const size_t off_status = lvi::align256(sizeof(Info));
        LVI_HIP(hipMemcpyAsync(d_in, h_in, up, hipMemcpyHostToDevice, stream));
        launch(reinterpret_cast<Info*>(d_out), reinterpret_cast<unsigned char*>(d_out + off_status));
        LVI_HIP(hipMemcpyAsync(h_out, d_out, off_status + (size_t)n, hipMemcpyDeviceToHost, stream));
        LVI_HIP(hipStreamSynchronize(stream));
        std::memcpy(status_out, h_out + off_status, (size_t)n);
        if (info_out) {
            std::memcpy(info_out, h_out, sizeof(Info));
            info_out->stream_us = stream_us;
        }
    }
};

}  // namespace lvi_ransac
#endif  // __HIPCC__
