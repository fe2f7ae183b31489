// Host-side mirror of the feature tracker's LiDAR depth association, over include/lvi_depth.h:
//
//   lidar_callback              feature_tracker_node.cpp:273-377   (window of clouds, fused depth cloud)
//   DepthRegister::get_depth    feature_tracker.h:116-331         (installed as FeatureTrackerNode::get_depth)
//
// The TF lookups of the reference (vins_world <- vins_body_ros at Time(0)) are the caller's: it hands the body pose to
// lidar_callback and, before each image, to set_image_pose (nullptr when the lookup failed).  Only liblvi_hip.so exports
// this ABI, so only code linked against it may include this header.
#pragma once
#include <memory>
#include <vector>

#include "../../include/lvi_depth.h"
#include "lvi_host.hpp"

namespace lvi_host {

// pose = (x, y, z, roll, pitch, yaw) of the body in the world frame
struct BodyPose { float v[6]; };

class DepthRegister {
public:
    DepthRegister(int device, int max_clouds, int max_cloud_points, int max_features, int lidar_skip, double window_s = 5.0)
        : max_features_(max_features)
    {
        check(lvi_depth_create(device, max_clouds, max_cloud_points, max_features, lidar_skip, window_s, &h_), "lvi_depth_create");
    }
    ~DepthRegister() { lvi_depth_destroy(h_); }
    DepthRegister(const DepthRegister&) = delete;
    DepthRegister& operator=(const DepthRegister&) = delete;
    lvi_depth* get() const { return h_; }

    // one cloud of point_cloud_topic; pose = nullptr when the TF lookup failed.  true when the cloud entered the window.
    bool lidar_callback(const std::vector<lvi_pt>& cloud, const BodyPose* pose, double stamp)
    {
        int32_t used = 0;
        check(lvi_depth_lidar_cloud(h_, cloud.empty() ? nullptr : cloud.data(), (int32_t)cloud.size(), pose ? pose->v : nullptr, stamp, &used),
              "lvi_depth_lidar_cloud");
        return used != 0;
    }
    // the transform get_depth's TF lookup would return for the next image (nullptr: the lookup failed)
    void set_image_pose(const BodyPose* pose)
    {
        have_pose_ = pose != nullptr;
        if (pose) pose_ = *pose;
    }
    // DepthRegister::get_depth for the published points (un_x, un_y, 1): the message's depth channel
    std::vector<float> get_depth(double /*stamp*/, const std::vector<Point3f>& features_2d)
    {
        std::vector<float> d(features_2d.size(), -1.f);
        if (features_2d.empty()) return d;
        if ((int)features_2d.size() > max_features_) throw Error(LVI_ERR_CAPACITY, "DepthRegister::get_depth: more features than max_features");
        static_assert(sizeof(Point3f) == 3 * sizeof(float), "Point3f must be three packed floats");
        check(lvi_depth_get(h_, have_pose_ ? pose_.v : nullptr, &features_2d[0].x, (int32_t)features_2d.size(), d.data()), "lvi_depth_get");
        return d;
    }
    // FeatureTrackerNode::get_depth := this register (the node's channel 5)
    void install(FeatureTrackerNode& node)
    {
        node.get_depth = [this](double stamp, const std::vector<Point3f>& f) { return get_depth(stamp, f); };
    }

private:
    lvi_depth* h_ = nullptr;
    int max_features_;
    bool have_pose_ = false;
    BodyPose pose_{};
};

}  // namespace lvi_host
