// Host-side mirror of rejectWithF's RANSAC over include/lvi_fmat.h:
//
//   cv::findFundamentalMat(un_cur_pts, un_forw_pts, cv::FM_RANSAC, F_THRESHOLD, 0.99, status)   feature_tracker.cpp:229
//
// installed as FeatureTracker::findFundamentalMat, as DepthRegister is installed as FeatureTrackerNode::get_depth.
// FeatureTracker's default stays "no hook, count a skip".  Only liblvi_hip.so exports this ABI, so only code linked
// against it may include this header.  Parity is against DESIGN §11's restatement of OpenCV 4.5.x, not OpenCV itself.
#pragma once
#include <vector>

#include "../../include/lvi_fmat.h"
#include "lvi_host.hpp"

namespace lvi_host {

class DeviceFundamental {
public:
    explicit DeviceFundamental(int device, int max_points = LVI_FMAT_MAX_POINTS, int max_iters = 1000) : max_points_(max_points)
    {
        check(lvi_fmat_create(device, max_points, max_iters, &h_), "lvi_fmat_create");
    }
    ~DeviceFundamental() { lvi_fmat_destroy(h_); }
    DeviceFundamental(const DeviceFundamental&) = delete;
    DeviceFundamental& operator=(const DeviceFundamental&) = delete;
    lvi_fmat* get() const { return h_; }

    // findFundamentalMat(a, b, FM_RANSAC, thr, 0.99, status): status is resized to a.size(); n < 7 leaves it all zeros
    // (the reference never calls with n < 8)
    void find(const std::vector<Point2f>& a, const std::vector<Point2f>& b, double thr, std::vector<uint8_t>& status, lvi_fmat_info* info = nullptr)
    {
        status.assign(a.size(), 0);
        if (a.size() < 7) return;
        if ((int)a.size() > max_points_) throw Error(LVI_ERR_CAPACITY, "DeviceFundamental::find: more points than max_points");
        static_assert(sizeof(Point2f) == 2 * sizeof(float), "Point2f must be two packed floats");
        check(lvi_fmat_find(h_, &a[0].x, &b[0].x, (int32_t)a.size(), thr, 0.99, status.data(), info), "lvi_fmat_find");
    }
    // FeatureTracker::findFundamentalMat := this RANSAC (rejectWithF of every later PUB frame)
    void install(FeatureTracker& ft)
    {
        ft.findFundamentalMat = [this](const std::vector<Point2f>& a, const std::vector<Point2f>& b, double thr, std::vector<uint8_t>& status) {
            find(a, b, thr, status);
        };
    }

private:
    lvi_fmat* h_ = nullptr;
    int max_points_;
};

}  // namespace lvi_host
