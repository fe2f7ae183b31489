// C entry points over the loop closer of the host mirror (lvi_loop_host.hpp): the loop-closure thread of a sequential
// mapOptimization node (lvh_seq), for replay harnesses that are not C++.  include/lvi_loop.h is exported by
// liblvi_hip.so only, so this file is linked into host/liblvi_host_hip.so alone (build.py).
#include <cstring>
#include <memory>

#include "lvi_loop_host.hpp"
#include "lvi_capi_util.hpp"

using namespace lvi_host;

extern "C" void* lvh_seq_node(struct lvh_seq* s);     // lvi_seq_capi.cpp
extern "C" lvi_lidar* lvh_seq_handle(struct lvh_seq* s);

struct lvh_loop {
    std::unique_ptr<LoopCloser> m;
};

extern "C" {

const char* lvh_loop_last_error(void) { return g_err.c_str(); }

// settings: frequency is the caller's (the thread's rate); the rest as params_lidar.yaml names them
lvh_loop* lvh_loop_create(lvh_seq* s, float search_radius, float search_time_diff, int32_t search_num, float fitness_score, float surf_leaf,
                          int32_t incremental_cloud)
{
    if (!s) { g_err = "null argument"; return nullptr; }
    LoopParams p;
    p.historyKeyframeSearchRadius = search_radius; p.historyKeyframeSearchTimeDiff = search_time_diff; p.historyKeyframeSearchNum = search_num;
    p.historyKeyframeFitnessScore = fitness_score; p.mappingSurfLeafSize = surf_leaf; p.incrementalCloud = incremental_cloud;
    lvh_loop* g = new lvh_loop();
    g->m.reset(new LoopCloser(*static_cast<const MapOptimizationNode*>(lvh_seq_node(s)), lvh_seq_handle(s), p));
    return g;
}

void lvh_loop_destroy(lvh_loop* g) { delete g; }

int32_t lvh_loop_reserve(lvh_loop* g, int32_t max_source_points, int32_t max_target_points)
{
    if (!g) return fail("null argument");
    return guarded([&]() -> int32_t { g->m->reserve(max_source_points, max_target_points); return LVI_OK; });
}

// loopInfoHandler: a message of n doubles
int32_t lvh_loop_info_msg(lvh_loop* g, const double* data, int32_t n)
{
    if (!g || (n > 0 && !data)) return fail("null argument");
    return guarded([&]() -> int32_t { g->m->loopInfoHandler(data, (size_t)n); return (int32_t)g->m->loopInfoVec.size(); });
}

// which: 0 = detectLoopClosureDistance, 1 = detectLoopClosureExternal, on fresh pose copies.  1 = found (keys[0] = cur, keys[1] = pre)
int32_t lvh_loop_detect(lvh_loop* g, int32_t which, double time_laser_info_cur, int32_t keys[2])
{
    if (!g || !keys) return fail("null argument");
    return guarded([&]() -> int32_t {
        g->m->copyKeyPoses();
        if (g->m->copy_cloudKeyPoses3D.empty()) return 0;
        int cur = -1, pre = -1;
        const bool ok = which ? g->m->detectLoopClosureExternal(&cur, &pre) : g->m->detectLoopClosureDistance(time_laser_info_cur, &cur, &pre);
        keys[0] = cur; keys[1] = pre;
        return ok ? 1 : 0;
    });
}

// startLoop / finishLoop: 1 = a job was enqueued / a constraint was pushed
int32_t lvh_loop_start(lvh_loop* g, double time_laser_info_cur)
{
    if (!g) return fail("null argument");
    return guarded([&]() -> int32_t { return g->m->startLoop(time_laser_info_cur) ? 1 : 0; });
}
int32_t lvh_loop_finish(lvh_loop* g, lvi_loop_info* info)
{
    if (!g) return fail("null argument");
    return guarded([&]() -> int32_t {
        const bool ok = g->m->finishLoop();
        if (info) *info = g->m->lastInfo;
        return ok ? 1 : 0;
    });
}

// the constraint queue: its length; pop the oldest (keys[2], between[16], *noise): 1 = popped, 0 = empty
int32_t lvh_loop_queue_size(lvh_loop* g) { return g ? (int32_t)g->m->loopQueue.size() : 0; }
int32_t lvh_loop_pop(lvh_loop* g, int32_t keys[2], double between[16], float* noise)
{
    if (!g || !keys || !between || !noise) return fail("null argument");
    if (g->m->loopQueue.empty()) return 0;
    const LoopConstraint c = g->m->loopQueue.front();
    g->m->loopQueue.pop_front();
    keys[0] = c.keyCur; keys[1] = c.keyPre; *noise = c.noise;
    std::memcpy(between, c.between, sizeof(c.between));
    return 1;
}

// loopIndexContainer as (cur, pre) pairs; *n = its size whatever capacity (in pairs) is
int32_t lvh_loop_closed(lvh_loop* g, int32_t* pairs, int32_t capacity, int32_t* n)
{
    if (!g || !n) return fail("null argument");
    *n = (int32_t)g->m->loopIndexContainer.size();
    if (pairs) {
        if (capacity < *n) return fail("capacity too small", LVI_ERR_CAPACITY);
        int i = 0;
        for (const auto& kv : g->m->loopIndexContainer) { pairs[2 * i] = kv.first; pairs[2 * i + 1] = kv.second; i++; }
    }
    return LVI_OK;
}

// the publishers' clouds of the last finished job (LVI_LOOP_TARGET = pubHistoryKeyFrames, LVI_LOOP_ALIGNED = pubIcpKeyFrames)
int32_t lvh_loop_cloud(lvh_loop* g, int32_t what, lvi_pt* out, int32_t capacity, int32_t* n)
{
    if (!g || !n) return fail("null argument");
    return guarded([&]() -> int32_t {
        *n = what == LVI_LOOP_TARGET ? g->m->lastInfo.n_target : g->m->lastInfo.n_source;
        if (out) {
            if (capacity < *n) return fail("capacity too small", LVI_ERR_CAPACITY);
            std::vector<lvi_pt> pts;
            g->m->fetch(what, pts);
            std::memcpy(out, pts.data(), sizeof(lvi_pt) * pts.size());
        }
        return LVI_OK;
    });
}

}  // extern "C"
