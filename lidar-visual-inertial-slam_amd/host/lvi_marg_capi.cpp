// C entry points over the marginalisation of the host mirror (lvi_marg_host.hpp): VinsMarginalizer, for replay harnesses
// that are not C++.  include/lvi_marg.h is exported by liblvi_hip.so only, so this file is linked into
// host/liblvi_host_hip.so alone (build.py), never into a host library built against the CPU oracle.
#include <cstring>

#include "lvi_marg_host.hpp"
#include "lvi_capi_util.hpp"

using namespace lvi_host;

extern "C" {

const char* lvh_marg_last_error(void) { return g_err.c_str(); }

// params may be NULL: lvi_marg_params_default
void* lvh_marg_create(int32_t device, int32_t max_features, int32_t estimate_td, const lvi_marg_params* params)
{
    try { return new VinsMarginalizer(device, max_features, estimate_td != 0, params); }
    catch (const std::exception& e) { g_err = e.what(); return nullptr; }
}

void lvh_marg_destroy(void* p) { delete static_cast<VinsMarginalizer*>(p); }

lvi_marg* lvh_marg_handle(void* p) { return p ? static_cast<VinsMarginalizer*>(p)->info.get() : nullptr; }

// vector2double: para_Pose [11][7], para_SpeedBias [11][9], para_Ex_Pose [7], para_Td
int32_t lvh_marg_set_window(void* p, const double* pose, const double* speed_bias, const double* ex_pose, double td)
{
    if (!p || !pose || !speed_bias || !ex_pose) return fail("null argument");
    VinsMarginalizer* v = static_cast<VinsMarginalizer*>(p);
    std::memcpy(v->paraPose, pose, sizeof(v->paraPose));
    std::memcpy(v->paraSpeedBias, speed_bias, sizeof(v->paraSpeedBias));
    std::memcpy(v->paraExPose, ex_pose, sizeof(v->paraExPose));
    v->paraTd = td;
    return LVI_OK;
}

// f_manager.feature: per feature its start_frame, its number of observations and its inverse depth; obs: every feature's
// observations in turn, 7 doubles each (point [3], velocity [2], cur_td, uv.y)
int32_t lvh_marg_set_features(void* p, int32_t count, const int32_t* start_frame, const int32_t* n_obs, const double* inv_dep, const double* obs)
{
    if (!p || (count > 0 && (!start_frame || !n_obs || !inv_dep || !obs)) || count < 0) return fail("bad argument");
    VinsMarginalizer* v = static_cast<VinsMarginalizer*>(p);
    v->features.clear();
    size_t at = 0;
    for (int f = 0; f < count; f++) {
        VinsFeature ft;
        ft.start_frame = start_frame[f]; ft.inv_dep = inv_dep[f];
        for (int k = 0; k < n_obs[f]; k++, at += 7) {
            VinsObservation o;
            std::memcpy(o.point, obs + at, sizeof(double) * 3);
            std::memcpy(o.velocity, obs + at + 3, sizeof(double) * 2);
            o.cur_td = obs[at + 5]; o.uv_y = obs[at + 6];
            ft.obs.push_back(o);
        }
        v->features.push_back(std::move(ft));
    }
    return LVI_OK;
}

// pre_integrations[1]->sum_dt and the evaluated IMUFactor (residual [15], jacobians 15x7, 15x9, 15x7, 15x9 in turn); residual
// NULL: no factor
int32_t lvh_marg_set_imu(void* p, double sum_dt, const double* residual, const double* jacobians)
{
    if (!p || (residual && !jacobians)) return fail("null argument");
    VinsMarginalizer* v = static_cast<VinsMarginalizer*>(p);
    v->hasImu = residual != nullptr; v->imuSumDt = sum_dt;
    if (residual) { std::memcpy(v->imuResidual, residual, sizeof(v->imuResidual)); std::memcpy(v->imuJacobians, jacobians, sizeof(v->imuJacobians)); }
    return LVI_OK;
}

// one pass through estimator.cpp:813-976; flag 0 MARGIN_OLD, 1 MARGIN_SECOND_NEW.  *ran: a marginalisation ran and its
// result is the prior.  Returns its status (LVI_OK or soft) or an error.
int32_t lvh_marg_run(void* p, int32_t flag, int32_t* ran, lvi_marg_info* info)
{
    if (!p || (flag != 0 && flag != 1)) return fail("bad argument");
    VinsMarginalizer* v = static_cast<VinsMarginalizer*>(p);
    return guarded([&]() -> int32_t {
        const bool r = v->run(flag == 0 ? VinsMarginalizer::MARGIN_OLD : VinsMarginalizer::MARGIN_SECOND_NEW);
        if (ran) *ran = r ? 1 : 0;
        if (info) *info = v->info.lastInfo;
        return r ? v->info.lastStatus : (v->info.lastStatus == LVI_MARG_NOT_FINITE ? LVI_MARG_NOT_FINITE : LVI_OK);
    });
}

}  // extern "C"
