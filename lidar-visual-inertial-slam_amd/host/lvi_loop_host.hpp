// Host mirror of mapOptimization's loop-closure thread over include/lvi_loop.h: loopInfoHandler (mapOptimization.cpp
// :537-547), detectLoopClosureExternal (:665-717), detectLoopClosureDistance (:630-663) and performLoopClosure (:549-628)
// up to the push onto loopIndexQueue / loopPoseQueue / loopNoiseQueue.  The submaps and the ICP run on the device; the
// constraint is computed here in the reference's precision.  Applying it (addLoopFactor, iSAM2, correctPoses) is the
// caller's: the odometry-chain node does not consume the queue.  Uses the HIP library only (the CPU oracle does not
// export lvi_loop_*).
#pragma once
#include <cmath>
#include <deque>
#include <map>
#include <utility>
#include <vector>

#include "../../include/lvi_loop.h"
#include "lvi_host.hpp"

namespace lvi_host {

struct LoopParams {                             // params_lidar.yaml:70-79 (utility.h:281-286)
    bool  loopClosureEnableFlag = true;
    float loopClosureFrequency = 1.0f;
    float historyKeyframeSearchRadius = 15.0f;
    float historyKeyframeSearchTimeDiff = 30.0f;
    int   historyKeyframeSearchNum = 25;
    float historyKeyframeFitnessScore = 0.3f;
    float mappingSurfLeafSize = 0.4f;           // downSizeFilterICP
    int   incrementalCloud = 1;                 // lvi_loop_params.incremental_cloud
};

// one entry of loopIndexQueue / loopPoseQueue / loopNoiseQueue
struct LoopConstraint {
    int32_t keyCur = -1, keyPre = -1;
    double between[16] = {};                    // poseFrom.between(poseTo), row-major 4x4
    float noise = 0.f;                          // the six variances of constraintNoise: the fitness score
};

// gtsam::Pose3(Rot3::RzRyRx(roll, pitch, yaw), Point3(x, y, z)) as a 4x4 double
inline void pose3Matrix(double roll, double pitch, double yaw, double x, double y, double z, double M[16])
{
    const double A = std::cos(yaw), B = std::sin(yaw), C = std::cos(pitch), D = std::sin(pitch), E = std::cos(roll), F = std::sin(roll);
    const double R[16] = {A * C, A * D * F - B * E, B * F + A * D * E, x,  B * C, A * E + B * D * F, B * D * E - A * F, y,  -D, C * F, C * E, z,  0, 0, 0, 1};
    for (int i = 0; i < 16; i++) M[i] = R[i];
}
// a.between(b) = a^-1 * b of two rigid 4x4 (the inverse of a rigid transform: R^T | -R^T t)
inline void pose3Between(const double a[16], const double b[16], double out[16])
{
    double inv[16] = {a[0], a[4], a[8], 0, a[1], a[5], a[9], 0, a[2], a[6], a[10], 0, 0, 0, 0, 1};
    for (int i = 0; i < 3; i++) inv[4 * i + 3] = -(inv[4 * i] * a[3] + inv[4 * i + 1] * a[7] + inv[4 * i + 2] * a[11]);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) out[4 * i + j] = inv[4 * i] * b[j] + inv[4 * i + 1] * b[4 + j] + inv[4 * i + 2] * b[8 + j] + inv[4 * i + 3] * b[12 + j];
}

// detectLoopClosureDistance (:630-663) on the pose copies.  radiusSearch returns its hits by ascending distance (ties by
// index): the first of them whose stamp lies more than historyKeyframeSearchTimeDiff from timeLaserInfoCur is the key to
// close with.
inline bool loopDetectDistance(const std::vector<lvi_pt>& poses3D, const std::vector<PointTypePose>& poses6D, const std::map<int, int>& loopIndexContainer,
                               const LoopParams& P, double timeLaserInfoCur, int* latestID, int* closestID)
{
    if (poses3D.empty()) return false;
    const int loopKeyCur = (int)poses3D.size() - 1;
    int loopKeyPre = -1;
    if (loopIndexContainer.find(loopKeyCur) != loopIndexContainer.end()) return false;
    for (const lvi_pt& hit : keyPosesWithin(poses3D, poses3D.back(), (double)P.historyKeyframeSearchRadius)) {
        const int id = (int)hit.intensity;
        if (std::abs(poses6D[id].time - timeLaserInfoCur) > P.historyKeyframeSearchTimeDiff) { loopKeyPre = id; break; }
    }
    if (loopKeyPre == -1 || loopKeyCur == loopKeyPre) return false;
    *latestID = loopKeyCur; *closestID = loopKeyPre;
    return true;
}

// detectLoopClosureExternal (:665-717) as written ("not used yet" in the reference: nothing publishes its topic)
inline bool loopDetectExternal(std::deque<std::pair<double, double>>& loopInfoVec, const std::vector<PointTypePose>& poses6D,
                               const std::map<int, int>& loopIndexContainer, const LoopParams& P, int* latestID, int* closestID)
{
    int loopKeyCur = -1, loopKeyPre = -1;
    if (loopInfoVec.empty()) return false;
    const double loopTimeCur = loopInfoVec.front().first, loopTimePre = loopInfoVec.front().second;
    loopInfoVec.pop_front();
    if (std::abs(loopTimeCur - loopTimePre) < P.historyKeyframeSearchTimeDiff) return false;
    const int cloudSize = (int)poses6D.size();
    if (cloudSize < 2) return false;
    loopKeyCur = cloudSize - 1;
    for (int i = cloudSize - 1; i >= 0; --i) {
        if (poses6D[i].time >= loopTimeCur) loopKeyCur = (int)std::round(poses6D[i].intensity);
        else break;
    }
    loopKeyPre = 0;
    for (int i = 0; i < cloudSize; ++i) {
        if (poses6D[i].time <= loopTimePre) loopKeyPre = (int)std::round(poses6D[i].intensity);
        else break;
    }
    if (loopKeyCur == loopKeyPre) return false;
    if (loopIndexContainer.find(loopKeyCur) != loopIndexContainer.end()) return false;
    *latestID = loopKeyCur; *closestID = loopKeyPre;
    return true;
}

class LoopCloser {
public:
    LoopCloser(const MapOptimizationNode& node, lvi_lidar* h, const LoopParams& p = LoopParams()) : P(p), node_(node), h_(h) {}
    LoopParams P;
    std::map<int, int> loopIndexContainer;                   // cur -> pre of every loop closed
    std::deque<std::pair<double, double>> loopInfoVec;       // (loopTimeCur, loopTimePre) of loopInfoHandler
    std::vector<lvi_pt> copy_cloudKeyPoses3D;
    std::vector<PointTypePose> copy_cloudKeyPoses6D;
    std::deque<LoopConstraint> loopQueue;                    // loopIndexQueue, loopPoseQueue, loopNoiseQueue in step
    lvi_loop_info lastInfo{};                                // of the last finished job

    // the arena of lvi_loop_start: the node reserves it once at start-up
    void reserve(int32_t max_source_points, int32_t max_target_points) { check(lvi_loop_reserve(h_, max_source_points, max_target_points), "lvi_loop_reserve"); }

    // loopInfoHandler (:537-547): messages of two values, the newest five kept
    void loopInfoHandler(const double* data, size_t n)
    {
        if (n != 2) return;
        loopInfoVec.push_back({data[0], data[1]});
        while (loopInfoVec.size() > 5) loopInfoVec.pop_front();
    }

    // the pose copies of :554-557 (the caller holds the node's mutex)
    void copyKeyPoses() { copy_cloudKeyPoses3D = node_.cloudKeyPoses3D; copy_cloudKeyPoses6D = node_.cloudKeyPoses6D; }

    bool detectLoopClosureDistance(double timeLaserInfoCur, int* latestID, int* closestID) const
    {
        return loopDetectDistance(copy_cloudKeyPoses3D, copy_cloudKeyPoses6D, loopIndexContainer, P, timeLaserInfoCur, latestID, closestID);
    }
    bool detectLoopClosureExternal(int* latestID, int* closestID)
    {
        return loopDetectExternal(loopInfoVec, copy_cloudKeyPoses6D, loopIndexContainer, P, latestID, closestID);
    }

    lvi_loop_params jobParams() const
    {
        lvi_loop_params p;
        lvi_loop_params_default(&p);
        p.search_num = P.historyKeyframeSearchNum;
        p.leaf = P.mappingSurfLeafSize;
        p.max_corr_dist = P.historyKeyframeSearchRadius * 2;
        p.incremental_cloud = P.incrementalCloud;
        return p;
    }

    // performLoopClosure :551-590 without the wait: the pose copies, the key search and the enqueue of the whole device job.
    // The caller holds the node's mutex for this call only (the store's poses are read at the enqueue).  false: no key poses
    // or no loop found.
    bool startLoop(double timeLaserInfoCur)
    {
        pending_ = false;
        if (node_.cloudKeyPoses3D.empty()) return false;
        copyKeyPoses();
        int cur, pre;
        if (!detectLoopClosureExternal(&cur, &pre))
            if (!detectLoopClosureDistance(timeLaserInfoCur, &cur, &pre)) return false;
        const lvi_loop_params p = jobParams();
        check(lvi_loop_start(h_, cur, pre, &p), "lvi_loop_start");
        pending_ = true; keyCur_ = cur; keyPre_ = pre;
        return true;
    }
    bool startLoop() { return startLoop(node_.laserTime()); }

    // :572-628 after the wait (may run beside the scan path): the gates, the fitness test, the constraint.  true: a constraint
    // was pushed onto loopQueue (the caller takes its lock round the push if another thread pops) and the loop recorded.
    bool finishLoop()
    {
        if (!pending_) return false;
        pending_ = false;
        check(lvi_loop_result(h_, &lastInfo), "lvi_loop_result");
        const lvi_loop_info& r = lastInfo;
        if (r.status == LVI_LOOP_TOO_FEW_POINTS) return false;                                   // :572-573
        if (!r.converged || r.fitness > (double)P.historyKeyframeFitnessScore) return false;     // :592-593
        loopQueue.push_back(constraintOf(r.transformation, copy_cloudKeyPoses6D[keyCur_], copy_cloudKeyPoses6D[keyPre_], keyCur_, keyPre_, r.fitness));
        loopIndexContainer[keyCur_] = keyPre_;
        return true;
    }
    bool performLoopClosure(double timeLaserInfoCur) { return startLoop(timeLaserInfoCur) && finishLoop(); }

    // :603-617.  correctionLidarFrame * tWrong and its Euler angles in f32 (Eigen::Affine3f, pcl::getTranslationAndEulerAngles),
    // the two gtsam poses and between() in double, noiseScore = (float) fitness
    static LoopConstraint constraintOf(const float correction[16], const PointTypePose& cur, const PointTypePose& pre, int keyCur, int keyPre, double fitness)
    {
        Affine3f corr;
        for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) corr.m[i][j] = correction[4 * i + j];
        const Affine3f tWrong = getTransformation(cur.x, cur.y, cur.z, cur.roll, cur.pitch, cur.yaw);      // pclPointToAffine3f
        float x, y, z, roll, pitch, yaw;
        getTranslationAndEulerAngles(affineMul(corr, tWrong), x, y, z, roll, pitch, yaw);
        double from[16], to[16];
        pose3Matrix(roll, pitch, yaw, x, y, z, from);
        pose3Matrix((double)pre.roll, (double)pre.pitch, (double)pre.yaw, (double)pre.x, (double)pre.y, (double)pre.z, to);   // pclPointTogtsamPose3
        LoopConstraint c;
        c.keyCur = keyCur; c.keyPre = keyPre;
        pose3Between(from, to, c.between);
        c.noise = (float)fitness;
        return c;
    }

    // the clouds of the two publishers: pubHistoryKeyFrames (:574-575, the target submap) and pubIcpKeyFrames (:596-601, the
    // source under the final transformation), of the last finished job
    void fetch(int32_t what, std::vector<lvi_pt>& out) const
    {
        out.resize(what == LVI_LOOP_TARGET ? lastInfo.n_target : lastInfo.n_source);
        check(lvi_loop_fetch(h_, what, 0, (int32_t)out.size(), out.data()), "lvi_loop_fetch");
    }

private:
    const MapOptimizationNode& node_;
    lvi_lidar* h_;
    bool pending_ = false;
    int keyCur_ = -1, keyPre_ = -1;
};

}  // namespace lvi_host
