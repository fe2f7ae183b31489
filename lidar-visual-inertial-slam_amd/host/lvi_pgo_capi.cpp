// C entry points over the pose-graph back end of the host mirror (lvi_pgo_host.hpp): PoseGraphBackend and the node's
// usePoseGraph hook, for replay harnesses that are not C++.  include/lvi_pgo.h is exported by liblvi_hip.so only, so this
// file is linked into host/liblvi_host_hip.so alone (build.py), never into a host library built against the CPU oracle.
#include <cstring>

#include "lvi_pgo_host.hpp"
#include "lvi_capi_util.hpp"

using namespace lvi_host;

extern "C" void* lvh_seq_node(struct lvh_seq* s);     // lvi_seq_capi.cpp

extern "C" {

const char* lvh_pgo_last_error(void) { return g_err.c_str(); }

// full_logmap < 0, max_iters <= 0 or conv_eps <= 0 keep that default of lvi_pgo_params_default
void* lvh_pgo_create(int32_t device, int32_t max_poses, int32_t max_loops, int32_t full_logmap, int32_t max_iters, double conv_eps)
{
    lvi_pgo_params p;
    lvi_pgo_params_default(&p);
    if (full_logmap >= 0) p.full_logmap = full_logmap;
    if (max_iters > 0) p.max_iters = max_iters;
    if (conv_eps > 0) p.conv_eps = conv_eps;
    try { return new PoseGraphBackend(device, max_poses, max_loops, &p); }
    catch (const std::exception& e) { g_err = e.what(); return nullptr; }
}

void lvh_pgo_destroy(void* p) { delete static_cast<PoseGraphBackend*>(p); }

lvi_pgo* lvh_pgo_handle(void* p) { return p ? static_cast<PoseGraphBackend*>(p)->get() : nullptr; }

// MapOptimizationNode::usePoseGraph on the node of lvh_seq_create; pg = NULL removes the hook.  The back end must outlive its use.
int32_t lvh_seq_use_pose_graph(lvh_seq* s, void* pg)
{
    if (!s) return fail("null argument");
    return guarded([&]() -> int32_t {
        static_cast<MapOptimizationNode*>(lvh_seq_node(s))->usePoseGraph(static_cast<PoseGraphBackend*>(pg));
        return LVI_OK;
    });
}

// one entry of loopIndexQueue / loopPoseQueue / loopNoiseQueue (what lvh_loop_pop hands out); returns the queue's length
int32_t lvh_pgo_push_loop(void* p, int32_t key_cur, int32_t key_pre, const double between[16], float noise)
{
    if (!p || !between) return fail("null argument");
    PoseGraphBackend* b = static_cast<PoseGraphBackend*>(p);
    LoopConstraint c;
    c.keyCur = key_cur; c.keyPre = key_pre; c.noise = noise;
    std::memcpy(c.between, between, sizeof(c.between));
    b->pushLoop(c);
    return (int32_t)b->loopQueue.size();
}

// counters [4]: updates, loops added, loops still queued, status of the last update; info and pose_to (the last
// addOdomFactor's poseTo) may be NULL
int32_t lvh_pgo_last(void* p, lvi_pgo_info* info, float pose_to[6], int32_t counters[4])
{
    if (!p) return fail("null argument");
    const PoseGraphBackend* b = static_cast<PoseGraphBackend*>(p);
    if (info) *info = b->lastInfo;
    if (pose_to) std::memcpy(pose_to, b->lastPoseTo, sizeof(b->lastPoseTo));
    if (counters) { counters[0] = b->updates; counters[1] = b->loopsAdded; counters[2] = (int32_t)b->loopQueue.size(); counters[3] = b->lastStatus; }
    return LVI_OK;
}

// MapOptimizationNode::useGps with the settings of utility.h:178-183
int32_t lvh_seq_use_gps(lvh_seq* s, int32_t use_gps_elevation, float gps_cov_threshold, float pose_cov_threshold)
{
    if (!s) return fail("null argument");
    return guarded([&]() -> int32_t {
        GpsSettings g;
        g.useGpsElevation = use_gps_elevation != 0; g.gpsCovThreshold = gps_cov_threshold; g.poseCovThreshold = pose_cov_threshold;
        static_cast<MapOptimizationNode*>(lvh_seq_node(s))->useGps(g);
        return LVI_OK;
    });
}

// gpsHandler (:334-337): the stamp, pose.pose.position and pose.covariance[0], [7], [14] of one message; returns the queue's length
int32_t lvh_seq_gps_push(lvh_seq* s, double stamp, const double xyz[3], const double cov_xyz[3])
{
    if (!s || !xyz || !cov_xyz) return fail("null argument");
    MapOptimizationNode* n = static_cast<MapOptimizationNode*>(lvh_seq_node(s));
    n->gpsHandler(stamp, xyz, cov_xyz);
    return (int32_t)n->gpsGate.gpsQueue.size();
}

// poseCovariance (:1591; row-major 6x6, may be NULL) and counters [3]: GPS factors added, messages still queued, GPS in use
int32_t lvh_seq_gps_last(lvh_seq* s, double cov[36], int32_t counters[3])
{
    if (!s) return fail("null argument");
    const MapOptimizationNode* n = static_cast<MapOptimizationNode*>(lvh_seq_node(s));
    if (cov) std::memcpy(cov, n->poseCovariance, sizeof(n->poseCovariance));
    if (counters) { counters[0] = n->gpsFactorsAdded; counters[1] = (int32_t)n->gpsGate.gpsQueue.size(); counters[2] = n->gpsInUse() ? 1 : 0; }
    return LVI_OK;
}

// MapOptimizationNode::posesCorrected / aLoopIsClosed
int32_t lvh_seq_poses_corrected(lvh_seq* s)
{
    if (!s) return fail("null argument");
    return static_cast<MapOptimizationNode*>(lvh_seq_node(s))->posesCorrected;
}

}  // extern "C"
