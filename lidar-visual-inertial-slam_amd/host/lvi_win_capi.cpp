// C entry points over the window optimisation of the host mirror (lvi_win_host.hpp): VinsWindowOptimizer, for replay
// harnesses that are not C++.  include/lvi_win.h is exported by liblvi_hip.so only, so this file is linked into
// host/liblvi_host_hip.so alone (build.py), never into a host library built against the CPU oracle.
#include <cstring>

#include "lvi_win_host.hpp"
#include "lvi_capi_util.hpp"

using namespace lvi_host;

extern "C" {

const char* lvh_win_last_error(void) { return g_err.c_str(); }

// marg: what lvh_marg_create returned; its window arrays are the ones optimised and it must outlive this object.
// params may be NULL: lvi_win_params_default
void* lvh_win_create(void* marg, int32_t device, int32_t max_features, int32_t estimate_extrinsic, int32_t num_iterations, double solver_time,
                     const lvi_win_params* params)
{
    if (!marg) { g_err = "null argument"; return nullptr; }
    try {
        VinsWindowOptimizer* v = new VinsWindowOptimizer(*static_cast<VinsMarginalizer*>(marg), device, max_features, params);
        v->estimateExtrinsic = estimate_extrinsic; v->numIterations = num_iterations; v->solverTime = solver_time;
        return v;
    } catch (const std::exception& e) { g_err = e.what(); return nullptr; }
}

void lvh_win_destroy(void* p) { delete static_cast<VinsWindowOptimizer*>(p); }

lvi_win* lvh_win_handle(void* p) { return p ? static_cast<VinsWindowOptimizer*>(p)->problem.get() : nullptr; }

// pre_integrations[j], j = 1..WINDOW_SIZE; rec NULL: no factor for that interval.  The ids of the record are ignored.
int32_t lvh_win_set_imu(void* p, int32_t j, const lvi_win_imu* rec)
{
    if (!p || j < 1 || j > VinsWindowOptimizer::WINDOW_SIZE) return fail("bad argument");
    VinsWindowOptimizer* v = static_cast<VinsWindowOptimizer*>(p);
    v->hasImu[j - 1] = rec != nullptr;
    if (rec) v->preIntegrations[j - 1] = *rec;
    return LVI_OK;
}

// lidar_depth_flag per feature of the marginaliser's feature list
int32_t lvh_win_set_lidar_flags(void* p, int32_t count, const int32_t* flags)
{
    if (!p || count < 0 || (count > 0 && !flags)) return fail("bad argument");
    VinsWindowOptimizer* v = static_cast<VinsWindowOptimizer*>(p);
    v->lidarDepthFlag.assign((size_t)count, 0);
    for (int k = 0; k < count; k++) v->lidarDepthFlag[k] = flags[k] != 0;
    return LVI_OK;
}

// estimator.cpp:696-811; flag 0 MARGIN_OLD, 1 MARGIN_SECOND_NEW (the time budget).  Returns the solve's status or an error.
int32_t lvh_win_optimize(void* p, int32_t flag, lvi_win_info* info)
{
    if (!p || (flag != 0 && flag != 1)) return fail("bad argument");
    VinsWindowOptimizer* v = static_cast<VinsWindowOptimizer*>(p);
    return guarded([&]() -> int32_t {
        const int32_t st = v->optimize(flag == 0 ? VinsMarginalizer::MARGIN_OLD : VinsMarginalizer::MARGIN_SECOND_NEW);
        if (info) *info = v->problem.lastInfo;
        return st;
    });
}

// double2vector's input: para_Pose [11][7], para_SpeedBias [11][9], para_Ex_Pose [7], para_Td, and the inverse depth of every
// feature of the list (cap entries at most; *count: the list's length)
int32_t lvh_win_get_window(void* p, double* pose, double* speed_bias, double* ex_pose, double* td, int32_t cap, int32_t* count, double* inv_dep)
{
    if (!p) return fail("null argument");
    const VinsMarginalizer& w = static_cast<VinsWindowOptimizer*>(p)->win;
    if (pose) std::memcpy(pose, w.paraPose, sizeof(w.paraPose));
    if (speed_bias) std::memcpy(speed_bias, w.paraSpeedBias, sizeof(w.paraSpeedBias));
    if (ex_pose) std::memcpy(ex_pose, w.paraExPose, sizeof(w.paraExPose));
    if (td) *td = w.paraTd;
    const int n = (int)w.features.size();
    if (count) *count = n;
    if (inv_dep) {
        if (cap < n) return fail("the array is shorter than the feature list", LVI_ERR_CAPACITY);
        for (int k = 0; k < n; k++) inv_dep[k] = w.features[k].inv_dep;
    }
    return LVI_OK;
}

}  // extern "C"
