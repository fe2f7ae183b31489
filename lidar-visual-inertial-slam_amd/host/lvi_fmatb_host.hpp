// Host-side mirror of rejectWithF's RANSAC for all cameras of a rig over include/lvi_fmatb.h:
//
//   cv::findFundamentalMat(un_cur_pts, un_forw_pts, cv::FM_RANSAC, F_THRESHOLD, 0.99, status)   feature_tracker.cpp:229
//
// once per camera that prepared (FeatureTrackerState::prepareRejectWithF), all in one call with one wait.  Installed with
// FeatureTrackerRig::useBatchedFundamental (host/lvi_tbatch_host.hpp).  Every camera's status equals what a DeviceFundamental
// (host/lvi_fmat_host.hpp) of its own returns.  Only liblvi_hip.so exports this ABI, so only code linked against it may
// include this header.
#pragma once
#include <vector>

#include "../../include/lvi_fmatb.h"
#include "lvi_host.hpp"

namespace lvi_host {

class BatchedFundamental {
public:
    BatchedFundamental(int device, int slots, int max_points = LVI_FMAT_MAX_POINTS, int max_iters = 1000) : slots_(slots), max_points_(max_points)
    {
        check(lvi_fmatb_create(device, slots, max_points, max_iters, &h_), "lvi_fmatb_create");
    }
    ~BatchedFundamental() { lvi_fmatb_destroy(h_); }
    BatchedFundamental(const BatchedFundamental&) = delete;
    BatchedFundamental& operator=(const BatchedFundamental&) = delete;
    lvi_fmatb* get() const { return h_; }
    int slots() const { return slots_; }

    // findFundamentalMat(*a[s], *b[s], FM_RANSAC, thresholds[s], 0.99, status[s]) for every slot with a[s] != nullptr; status[s] is
    // resized to a[s]->size() (n < 7 leaves it all zeros: the reference never calls with n < 8).  A slot with a[s] == nullptr sits
    // out and its status[s] is left alone.
    void find(const std::vector<const std::vector<Point2f>*>& a, const std::vector<const std::vector<Point2f>*>& b, const std::vector<double>& thresholds,
              std::vector<std::vector<uint8_t>>& status, lvi_fmat_info* info = nullptr)
    {
        const size_t S = (size_t)slots_;
        if (a.size() != S || b.size() != S || thresholds.size() != S) throw Error(LVI_ERR_INVALID_ARG, "BatchedFundamental::find: one entry per slot");
        static_assert(sizeof(Point2f) == 2 * sizeof(float), "Point2f must be two packed floats");
        status.resize(S);
        const float *p1[LVI_TRACKER_MAX_BATCH], *p2[LVI_TRACKER_MAX_BATCH];
        uint8_t* st[LVI_TRACKER_MAX_BATCH];
        int32_t n[LVI_TRACKER_MAX_BATCH];
        bool any = false;
        for (size_t s = 0; s < S; s++) {
            p1[s] = p2[s] = nullptr; st[s] = nullptr; n[s] = -1;
            if (!a[s] || !b[s]) continue;
            if (a[s]->size() != b[s]->size()) throw Error(LVI_ERR_INVALID_ARG, "BatchedFundamental::find: the point sets of a slot differ in length");
            status[s].assign(a[s]->size(), 0);
            if (a[s]->size() < 7) continue;
            if ((int)a[s]->size() > max_points_) throw Error(LVI_ERR_CAPACITY, "BatchedFundamental::find: more points than max_points");
            p1[s] = &(*a[s])[0].x; p2[s] = &(*b[s])[0].x; st[s] = status[s].data(); n[s] = (int32_t)a[s]->size();
            any = true;
        }
        if (!any && !info) return;
        check(lvi_fmatb_find(h_, p1, p2, n, thresholds.data(), 0.99, st, info), "lvi_fmatb_find");
    }
    // lvi_fmatb_find calls with at least one active slot, since creation
    int64_t calls() const
    {
        int64_t c = 0;
        check(lvi_fmatb_counters(h_, &c, nullptr, nullptr, nullptr), "lvi_fmatb_counters");
        return c;
    }

private:
    lvi_fmatb* h_ = nullptr;
    int slots_, max_points_;
};

}  // namespace lvi_host
