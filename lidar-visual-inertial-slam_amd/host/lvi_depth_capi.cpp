// C entry points over the depth register of the host mirror (lvi_depth_host.hpp): the feature tracker node's lidar
// callback and its get_depth hook, for replay harnesses that are not C++.  include/lvi_depth.h is exported by
// liblvi_hip.so only, so this file is linked into host/liblvi_host_hip.so alone (build.py), never into a host library
// built against the CPU oracle; lvi_seq_capi.cpp stays free of it.
#include <memory>

#include "lvi_depth_host.hpp"
#include "lvi_capi_util.hpp"

using namespace lvi_host;

extern "C" void* lvh_trk_node(struct lvh_trk* t);     // lvi_seq_capi.cpp

struct lvh_depth {
    std::unique_ptr<DepthRegister> reg;
};

extern "C" {

const char* lvh_depth_last_error(void) { return g_err.c_str(); }

lvh_depth* lvh_depth_create(int32_t device, int32_t max_clouds, int32_t max_cloud_points, int32_t max_features, int32_t lidar_skip, double window_s)
{
    lvh_depth* d = new lvh_depth();
    const int32_t st = guarded([&]() -> int32_t {
        d->reg.reset(new DepthRegister(device, max_clouds, max_cloud_points, max_features, lidar_skip, window_s));
        return LVI_OK;
    });
    if (st != LVI_OK) { delete d; return nullptr; }
    return d;
}
void lvh_depth_destroy(lvh_depth* d) { delete d; }
lvi_depth* lvh_depth_handle(lvh_depth* d) { return d ? d->reg->get() : nullptr; }

// FeatureTrackerNode::get_depth := the register (channel 5 of every message lvh_trk_image assembles from now on)
int32_t lvh_depth_install(lvh_depth* d, struct lvh_trk* t)
{
    if (!d || !t) return fail("null argument");
    d->reg->install(*static_cast<FeatureTrackerNode*>(lvh_trk_node(t)));
    return LVI_OK;
}

// lidar_callback: pose6 = (x, y, z, roll, pitch, yaw) or NULL (no TF)
int32_t lvh_depth_lidar(lvh_depth* d, const lvi_pt* pts, int32_t n, const float* pose6, double stamp, int32_t* used)
{
    if (!d || n < 0 || (n > 0 && !pts)) return fail("bad arguments");
    return guarded([&]() -> int32_t {
        BodyPose p{};
        if (pose6) for (int k = 0; k < 6; k++) p.v[k] = pose6[k];
        const bool u = d->reg->lidar_callback(std::vector<lvi_pt>(pts, pts + n), pose6 ? &p : nullptr, stamp);
        if (used) *used = u ? 1 : 0;
        return LVI_OK;
    });
}

// the pose get_depth's TF lookup returns for the next image (NULL: the lookup fails)
int32_t lvh_depth_set_image_pose(lvh_depth* d, const float* pose6)
{
    if (!d) return fail("null argument");
    BodyPose p{};
    if (pose6) for (int k = 0; k < 6; k++) p.v[k] = pose6[k];
    d->reg->set_image_pose(pose6 ? &p : nullptr);
    return LVI_OK;
}

}  // extern "C"
