// The host half of lvi_pnp_solve (include/lvi_pnp.h): the sample stream of cv::solvePnPRansac's RANSAC and
// the iteration-count table.  No HIP in here: tests compile it with a stand-alone main under the host sanitizers.
//
//   cv::RNG((uint64)-1)                              multiply-with-carry, as ptsetreg.cpp seeds it
//   RANSACPointSetRegistrator::getSubset             modelPoints = 5: distinct indices, a duplicate is redrawn; the PnP
//                                                    callback has no checkSubset, so the first five distinct draws are
//                                                    the subset and getSubset never fails
//   RANSACUpdateNumIters(p, ep, 5, niters)           log(1 - (1 - ep)^5) per possible inlier count, so the device walk
//                                                    never calls log or pow
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

namespace lvi_pnp_stream {

constexpr int MODEL_POINTS = 5;

struct CvRng {
    uint64_t s = ~(uint64_t)0;
    uint32_t next() { s = (uint64_t)(uint32_t)s * 4164903690u + (uint32_t)(s >> 32); return (uint32_t)s; }
    int uniform(int a, int b) { return a == b ? a : (int)(next() % (uint32_t)(b - a) + (uint32_t)a); }
};

// one subset of five distinct indices in [0, n); n >= 5 or the redraw never ends
inline void get_subset(CvRng& rng, int n, int32_t* idx)
{
    for (int i = 0; i < MODEL_POINTS; ++i) {
        int k = rng.uniform(0, n);
        while (std::find(idx, idx + i, k) != idx + i) k = rng.uniform(0, n);
        idx[i] = k;
    }
}

// subsets [count][5]: the whole stream of one call (the draws never depend on a model); returns count, 0 when n < 5
inline int sample_stream(int n, int count, int32_t* subsets)
{
    if (n < MODEL_POINTS || count < 0) return 0;
    CvRng rng;
    for (int h = 0; h < count; ++h) get_subset(rng, n, subsets + MODEL_POINTS * h);
    return count;
}

// log(1 - (1 - ep)^5) for ep = (n - good) / n; +inf marks denom < DBL_MIN (RANSACUpdateNumIters returns 0 there)
inline double update_log(int n, int good)
{
    double ep = (double)(n - good) / n;
    ep = std::max(ep, 0.); ep = std::min(ep, 1.);
    const double denom = 1. - std::pow(1. - ep, MODEL_POINTS);
    if (denom < DBL_MIN) return HUGE_VAL;
    return std::log(denom);
}

// logtab [n + 1]
inline void update_log_table(int n, double* logtab)
{
    for (int g = 0; g <= n; ++g) logtab[g] = update_log(n, g);
}

}  // namespace lvi_pnp_stream
