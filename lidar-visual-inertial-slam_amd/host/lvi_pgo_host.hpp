// Host mirror of mapOptimization's factor graph over include/lvi_pgo.h: what the node's saveKeyFramesAndFactor and
// correctPoses call (lvi_host::PoseGraphHook of lvi_host.hpp):
//
//   addOdomFactor   mapOptimization.cpp:1414-1428   the prior of key 0, BetweenFactor(n - 1, n, poseFrom.between(poseTo))
//   addLoopFactor   :1509-1527                      the constraints of loopIndexQueue / loopPoseQueue / loopNoiseQueue
//   update          :1546-1566                      isam->update (2, or 7 after a loop) + calculateEstimate, as the minimiser
//   estimate        :1567-1599, :1627-1640          isamCurrentEstimate.at<Pose3>(i) as (roll, pitch, yaw, x, y, z) floats
//
// The caller moves what LoopCloser::loopQueue holds into pushLoop / takeLoops (under its queue lock), as the reference's
// loop thread fills the three queues.  GPS: addGpsFactor (the GPSFactor of :1497-1499) and marginalCovariance (:1591) over
// include/lvi_pgo_gps.h; the decisions of addGPSFactor are the node's GpsGate (lvi_gps_gate.hpp).  Only liblvi_hip.so exports this ABI, so only code
// linked against it may include this header.  Parity is with the minimiser of the graph's cost, not with
// iSAM2's iterate.
#pragma once
#include <deque>

#include "../../include/lvi_pgo.h"
#include "../../include/lvi_pgo_gps.h"
#include "lvi_loop_host.hpp"

namespace lvi_host {

class PoseGraphBackend : public PoseGraphHook {
public:
    PoseGraphBackend(int device, int max_poses, int max_loops, const lvi_pgo_params* p = nullptr)
    {
        check(lvi_pgo_create(device, max_poses, max_loops, &g_), "lvi_pgo_create");
        if (p && lvi_pgo_set_params(g_, p) < 0) { const Error e(LVI_ERR_INVALID_ARG, "lvi_pgo_set_params"); lvi_pgo_destroy(g_); throw e; }
    }
    ~PoseGraphBackend() override { lvi_pgo_destroy(g_); }
    PoseGraphBackend(const PoseGraphBackend&) = delete;
    PoseGraphBackend& operator=(const PoseGraphBackend&) = delete;
    lvi_pgo* get() const { return g_; }

    std::deque<LoopConstraint> loopQueue;        // pushed by the caller, drained by addLoopFactor
    lvi_pgo_info lastInfo{};                     // of the last update
    int32_t lastStatus = LVI_OK;                 // LVI_OK or LVI_PGO_NOT_CONVERGED
    int updates = 0, loopsAdded = 0, gpsAdded = 0;
    float lastPoseTo[6] = {};                    // poseTo of the last addOdomFactor

    void pushLoop(const LoopConstraint& c) { loopQueue.push_back(c); }
    void takeLoops(std::deque<LoopConstraint>& q) { while (!q.empty()) { loopQueue.push_back(q.front()); q.pop_front(); } }

    int size() const override
    {
        int32_t n = 0;
        check(lvi_pgo_count(g_, &n, nullptr), "lvi_pgo_count");
        return n;
    }
    void addOdomFactor(const float* poseFrom, const float poseTo[6]) override
    {
        check(lvi_pgo_add_pose(g_, poseFrom, poseTo, nullptr), "lvi_pgo_add_pose");
        for (int k = 0; k < 6; k++) lastPoseTo[k] = poseTo[k];
    }
    // :1511-1526: every queued constraint becomes BetweenFactor(cur, pre, poseBetween) with the fitness score as its six variances
    int addLoopFactor() override
    {
        int n = 0;
        while (!loopQueue.empty()) {
            const LoopConstraint& c = loopQueue.front();
            check(lvi_pgo_add_loop(g_, c.keyCur, c.keyPre, c.between, c.noise), "lvi_pgo_add_loop");
            loopQueue.pop_front();
            n++;
        }
        loopsAdded += n;
        return n;
    }
    void update() override
    {
        lastStatus = check(lvi_pgo_solve(g_, &lastInfo), "lvi_pgo_solve");
        updates++;
    }
    void addGpsFactor(int key, const float xyz[3], const float variance[3]) override
    {
        check(lvi_pgo_gps_add(g_, key, xyz, variance), "lvi_pgo_gps_add");
        gpsAdded++;
    }
    bool marginalCovariance(int key, double cov[36]) override
    {
        check(lvi_pgo_gps_marginal_covariance(g_, key, cov), "lvi_pgo_gps_marginal_covariance");
        return true;
    }
    void estimate(int first, int count, float* rpyxyz) override { check(lvi_pgo_get_poses(g_, first, count, nullptr, rpyxyz), "lvi_pgo_get_poses"); }

private:
    lvi_pgo* g_ = nullptr;
};

}  // namespace lvi_host
