// C entry points over the feature manager of the host mirror (lvi_fman_host.hpp): FeatureManager, for replay harnesses that
// are not C++.  include/lvi_fman.h is exported by liblvi_hip.so only, so this file is linked into host/liblvi_host_hip.so
// alone (build.py), never into a host library built against the CPU oracle.

#include "lvi_fman_host.hpp"
#include "lvi_capi_util.hpp"

using namespace lvi_host;

extern "C" {

const char* lvh_fman_last_error(void) { return g_err.c_str(); }

// params may be NULL: lvi_fman_params_default
void* lvh_fman_create(int32_t device, int32_t max_features, const lvi_fman_params* params)
{
    try { return new FeatureManager(device, max_features, params); }
    catch (const std::exception& e) { g_err = e.what(); return nullptr; }
}

void lvh_fman_destroy(void* p) { delete static_cast<FeatureManager*>(p); }

lvi_fman* lvh_fman_handle(void* p) { return p ? static_cast<FeatureManager*>(p)->get() : nullptr; }

int32_t lvh_fman_clear_state(void* p)
{
    if (!p) return fail("null argument");
    return guarded([&]() -> int32_t { static_cast<FeatureManager*>(p)->clearState(); return LVI_OK; });
}

// addFeatureCheckParallax -> 1 (MARGIN_OLD), 0 (MARGIN_SECOND_NEW) or an error; info may be NULL
int32_t lvh_fman_add_frame(void* p, int32_t frame_count, int32_t n, const int32_t* ids, const double* obs, double td, lvi_fman_frame_info* info)
{
    if (!p) return fail("null argument");
    FeatureManager* m = static_cast<FeatureManager*>(p);
    return guarded([&]() -> int32_t {
        const bool key = m->addFeatureCheckParallax(frame_count, n, ids, obs, td);
        if (info) *info = m->lastFrame;
        return key ? 1 : 0;
    });
}

int32_t lvh_fman_triangulate(void* p, const double* Ps, const double* Rs, const double* tic, const double* ric, lvi_fman_tri_info* info)
{
    if (!p) return fail("null argument");
    FeatureManager* m = static_cast<FeatureManager*>(p);
    return guarded([&]() -> int32_t {
        m->triangulate(Ps, Rs, tic, ric);
        if (info) *info = m->lastTri;
        return LVI_OK;
    });
}

// marg, win: what lvh_marg_create and lvh_win_create returned
int32_t lvh_fman_fill_window(void* p, void* marg, void* win)
{
    if (!p || !marg || !win) return fail("null argument");
    return guarded([&]() -> int32_t {
        static_cast<FeatureManager*>(p)->fillWindow(*static_cast<VinsMarginalizer*>(marg), *static_cast<VinsWindowOptimizer*>(win));
        return LVI_OK;
    });
}

int32_t lvh_fman_take_depths(void* p, void* marg)
{
    if (!p || !marg) return fail("null argument");
    return guarded([&]() -> int32_t { static_cast<FeatureManager*>(p)->takeDepths(*static_cast<VinsMarginalizer*>(marg)); return LVI_OK; });
}

int32_t lvh_fman_remove_failures(void* p)
{
    if (!p) return fail("null argument");
    return guarded([&]() -> int32_t { static_cast<FeatureManager*>(p)->removeFailures(); return LVI_OK; });
}

// slideWindowOld (estimator.cpp:1082-1099); shift_depth 0: removeBack, the pose arguments may be NULL
int32_t lvh_fman_slide_old(void* p, int32_t shift_depth, const double* back_R0, const double* back_P0, const double* Rs0, const double* Ps0, const double* ric,
                           const double* tic)
{
    if (!p || (shift_depth && (!back_R0 || !back_P0 || !Rs0 || !Ps0 || !ric || !tic))) return fail("null argument");
    return guarded([&]() -> int32_t {
        static_cast<FeatureManager*>(p)->slideWindowOld(shift_depth != 0, back_R0, back_P0, Rs0, Ps0, ric, tic);
        return LVI_OK;
    });
}

// slideWindowNew (estimator.cpp:1076-1080)
int32_t lvh_fman_slide_new(void* p, int32_t frame_count)
{
    if (!p) return fail("null argument");
    return guarded([&]() -> int32_t { static_cast<FeatureManager*>(p)->slideWindowNew(frame_count); return LVI_OK; });
}

}  // extern "C"
