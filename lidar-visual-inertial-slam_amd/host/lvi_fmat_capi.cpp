// C entry point over the device RANSAC of the host mirror (lvi_fmat_host.hpp): rejectWithF's findFundamentalMat hook,
// for replay harnesses that are not C++.  include/lvi_fmat.h is exported by liblvi_hip.so only, so this file is linked
// into host/liblvi_host_hip.so alone (build.py), never into a host library built against the CPU oracle.
#include <memory>

#include "lvi_fmat_host.hpp"
#include "lvi_capi_util.hpp"

using namespace lvi_host;

extern "C" void* lvh_trk_node(struct lvh_trk* t);     // lvi_seq_capi.cpp

extern "C" {

const char* lvh_fmat_last_error(void) { return g_err.c_str(); }

// FeatureTracker::findFundamentalMat := a DeviceFundamental on `device` owned by the tracker's hook (it lives as long as
// the hook: until the hook is replaced or the tracker destroyed)
int32_t lvh_trk_use_device_fundamental(struct lvh_trk* t, int32_t device)
{
    if (!t) return fail("null argument");
    return guarded([&]() -> int32_t {
        auto df = std::make_shared<DeviceFundamental>(device);
        FeatureTracker* ft = &static_cast<FeatureTrackerNode*>(lvh_trk_node(t))->trackerData;
        ft->findFundamentalMat = [df](const std::vector<Point2f>& a, const std::vector<Point2f>& b, double thr, std::vector<uint8_t>& status) {
            df->find(a, b, thr, status);
        };
        return LVI_OK;
    });
}

}  // extern "C"
