// C entry points over the global mapper of the host mirror (lvi_gmap_host.hpp): publishGlobalMap and save_map of a
// sequential mapOptimization node (lvh_seq), for replay harnesses that are not C++.  include/lvi_gmap.h is exported by
// liblvi_hip.so only, so this file is linked into host/liblvi_host_hip.so alone (build.py).
#include <cstring>
#include <memory>

#include "lvi_gmap_host.hpp"
#include "lvi_capi_util.hpp"

using namespace lvi_host;

extern "C" void* lvh_seq_node(struct lvh_seq* s);     // lvi_seq_capi.cpp
extern "C" lvi_lidar* lvh_seq_handle(struct lvh_seq* s);

struct lvh_gmap {
    std::unique_ptr<GlobalMapper> m;
    std::vector<lvi_pt> last;                           // the last published cloud
};

extern "C" {

const char* lvh_gmap_last_error(void) { return g_err.c_str(); }

lvh_gmap* lvh_gmap_create(lvh_seq* s, float search_radius, float pose_density, float leaf_size)
{
    if (!s) { g_err = "null argument"; return nullptr; }
    GlobalMapParams p;
    p.globalMapVisualizationSearchRadius = search_radius; p.globalMapVisualizationPoseDensity = pose_density; p.globalMapVisualizationLeafSize = leaf_size;
    lvh_gmap* g = new lvh_gmap();
    g->m.reset(new GlobalMapper(*static_cast<const MapOptimizationNode*>(lvh_seq_node(s)), lvh_seq_handle(s), p));
    return g;
}

void lvh_gmap_destroy(lvh_gmap* g) { delete g; }

int32_t lvh_gmap_reserve(lvh_gmap* g, int32_t max_points)
{
    if (!g) return fail("null argument");
    return guarded([&]() -> int32_t { g->m->reserve(max_points); return LVI_OK; });
}

// steps 2-6: the fuse order of the key clouds; *n = its length whatever capacity is
int32_t lvh_gmap_keys(lvh_gmap* g, int32_t* keys, int32_t capacity, int32_t* n)
{
    if (!g || !n) return fail("null argument");
    return guarded([&]() -> int32_t {
        const std::vector<int32_t> k = g->m->globalMapKeys();
        *n = (int32_t)k.size();
        if (keys) { if (capacity < *n) return fail("capacity too small", LVI_ERR_CAPACITY); std::memcpy(keys, k.data(), sizeof(int32_t) * k.size()); }
        return LVI_OK;
    });
}

// publishGlobalMap: 1 = published (info = n_fused, n_out, overflow, filtered), 0 = no key poses
int32_t lvh_gmap_publish(lvh_gmap* g, int32_t info[4])
{
    if (!g || !info) return fail("null argument");
    return guarded([&]() -> int32_t {
        lvi_gmap_info r{};
        if (!g->m->publishGlobalMap(g->last, &r)) { g->last.clear(); return 0; }
        info[0] = r.n_fused; info[1] = r.n_out; info[2] = r.overflow; info[3] = r.filtered;
        return 1;
    });
}

// the last published cloud; *n = its size whatever capacity is
int32_t lvh_gmap_cloud(lvh_gmap* g, lvi_pt* out, int32_t capacity, int32_t* n)
{
    if (!g || !n) return fail("null argument");
    *n = (int32_t)g->last.size();
    if (out) { if (capacity < *n) return fail("capacity too small", LVI_ERR_CAPACITY); std::memcpy(out, g->last.data(), sizeof(lvi_pt) * g->last.size()); }
    return LVI_OK;
}

// the save_map service: 1 = success (the GlobalMap write), 0 = failure
int32_t lvh_gmap_save(lvh_gmap* g, const char* dir, float resolution)
{
    if (!g || !dir) return fail("null argument");
    return guarded([&]() -> int32_t { return g->m->saveMap(dir, resolution) ? 1 : 0; });
}

}  // extern "C"
