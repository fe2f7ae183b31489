// Host-side mirror of the pose_graph KeyFrame's loop confirmation over include/lvi_pnp.h:
//
//   KeyFrame::PnPRANSAC          keyframe.cpp:135-176   cv::solvePnPRansac(matched_3d, matched_2d_old_norm, K = I, D, rvec, t,
//                                                       true, 100, 10.0 / 460.0, 0.99, inliers) -> status     -> PnPRansac::status
//   KeyFrame::findConnection     keyframe.cpp:179-211   searchByBRIEFDes, the six reduceVector calls, the > MIN_LOOP_NUM
//                                                       gate, PnPRANSAC, six more, the second gate          -> findConnection
//
// findConnection reads only the inlier set of solvePnPRansac: rvec and t are never used afterwards, so the initial guess
// built from origin_vio_R / origin_vio_T (:144-152) is not an input here.  What follows the second gate (the match image,
// :213-250) stays with the caller.  Only liblvi_hip.so exports this ABI, so only code linked against it may include this
// header.  Parity is against DESIGN §16's restatement of OpenCV 4.5.x, not OpenCV itself.
#pragma once
#include <vector>

#include "../../include/lvi_pnp.h"
#include "lvi_kf_host.hpp"

namespace lvi_host {

class PnPRansac {
public:
    explicit PnPRansac(int device, int max_points = LVI_PNP_MAX_POINTS, int max_iters = 100) : max_points_(max_points)
    {
        check(lvi_pnp_create(device, max_points, max_iters, &h_), "lvi_pnp_create");
    }
    ~PnPRansac() { lvi_pnp_destroy(h_); }
    PnPRansac(const PnPRansac&) = delete;
    PnPRansac& operator=(const PnPRansac&) = delete;
    lvi_pnp* get() const { return h_; }

    // keyframe.cpp:163-174: the status vector PnPRANSAC leaves, one byte per correspondence
    std::vector<uint8_t> status(const std::vector<Point2f>& matched_2d_old_norm, const std::vector<Point3f>& matched_3d, lvi_pnp_info* info = nullptr)
    {
        static_assert(sizeof(Point2f) == 2 * sizeof(float) && sizeof(Point3f) == 3 * sizeof(float), "Point2f / Point3f must be packed floats");
        if (matched_2d_old_norm.size() != matched_3d.size()) throw Error(LVI_ERR_INVALID_ARG, "PnPRansac::status: the vectors differ in length");
        if ((int)matched_3d.size() > max_points_) throw Error(LVI_ERR_CAPACITY, "PnPRansac::status: more points than max_points");
        std::vector<uint8_t> st(matched_3d.size(), 0);
        // the `float reprojectionError` parameter receives the double 10.0 / 460.0
        check(lvi_pnp_solve(h_, matched_3d.empty() ? nullptr : &matched_3d[0].x, matched_3d.empty() ? nullptr : &matched_2d_old_norm[0].x, (int32_t)matched_3d.size(),
                            (double)(float)(10.0 / 460.0), 0.99, st.data(), info), "lvi_pnp_solve");
        return st;
    }

private:
    lvi_pnp* h_ = nullptr;
    int max_points_;
};

// KeyFrame::findConnection (keyframe.cpp:179-211) up to its return value: true = the match message would be published
// (loop_detector.cpp:29).  c.front_3d / c.front_2d_old_norm keep what PnPRANSAC received, c.pnp_status what it answered.
inline bool findConnection(KeyFrameDescriber& kd, PnPRansac& pnp, const KeyFrame& cur, const KeyFrame& old_kf, Connection& c)
{
    c.pnp_status.clear(); c.front_3d.clear(); c.front_2d_old_norm.clear();
    if (!kd.findConnectionFront(cur, old_kf, c)) return false;
    c.front_3d = c.matched_3d;
    c.front_2d_old_norm = c.matched_2d_old_norm;
    c.pnp_status = pnp.status(c.matched_2d_old_norm, c.matched_3d);
    KeyFrameDescriber::reduceVector(c.matched_2d_cur, c.pnp_status);
    KeyFrameDescriber::reduceVector(c.matched_2d_old, c.pnp_status);
    KeyFrameDescriber::reduceVector(c.matched_2d_cur_norm, c.pnp_status);
    KeyFrameDescriber::reduceVector(c.matched_2d_old_norm, c.pnp_status);
    KeyFrameDescriber::reduceVector(c.matched_3d, c.pnp_status);
    KeyFrameDescriber::reduceVector(c.matched_id, c.pnp_status);
    return (int)c.matched_2d_cur.size() > MIN_LOOP_NUM;
}

}  // namespace lvi_host
