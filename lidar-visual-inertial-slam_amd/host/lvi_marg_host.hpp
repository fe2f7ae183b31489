// Host mirror of vins_estimator's marginalisation over include/lvi_marg.h:
//
//   MarginalizationInfo   marginalization_factor.cpp:89-129, 174-318   addResidualBlockInfo / preMarginalize / marginalize /
//                                                                       getParameterBlocks, with ids for addresses
//   VinsMarginalizer      estimator.cpp:813-976                         the MARGIN_OLD and MARGIN_SECOND_NEW branches of
//                                                                       Estimator::optimization over the window arrays
//
// The prior stays on the device between calls.  A node that keeps Ceres for the window optimisation reads it back with
// MarginalizationInfo::prior (lvi_marg_get_prior) and the layout, and evaluates its MarginalizationFactor from them.
// IMUFactor is not restated: the caller hands it in evaluated (setImu), or not at all.  Only liblvi_hip.so exports this
// ABI, so only code linked against it may include this header.
#pragma once
#include <algorithm>
#include <vector>

#include "../../include/lvi_marg.h"
#include "lvi_host.hpp"

namespace lvi_host {

class MarginalizationInfo {
public:
    MarginalizationInfo(int device, const lvi_marg_caps& caps, const lvi_marg_params* p = nullptr)
    {
        check(lvi_marg_create(device, &caps, &m_), "lvi_marg_create");
        if (p && lvi_marg_set_params(m_, p) < 0) { const Error e(LVI_ERR_INVALID_ARG, "lvi_marg_set_params"); lvi_marg_destroy(m_); throw e; }
    }
    ~MarginalizationInfo() { lvi_marg_destroy(m_); }
    MarginalizationInfo(const MarginalizationInfo&) = delete;
    MarginalizationInfo& operator=(const MarginalizationInfo&) = delete;
    lvi_marg* get() const { return m_; }

    lvi_marg_info lastInfo{};
    int32_t lastStatus = LVI_OK;
    bool valid = false;                                  // the reference's last_marginalization_info != nullptr
    std::vector<int32_t> keepIds, keepSizes, keepIdx;    // last_marginalization_parameter_blocks, keep_block_size, keep_block_idx

    void begin() { check(lvi_marg_begin(m_), "lvi_marg_begin"); }
    void setBlock(int32_t id, int32_t size, const double* v) { check(lvi_marg_set_block(m_, id, size, v), "lvi_marg_set_block"); }
    void addProjection(const std::vector<lvi_marg_projection>& r)
    {
        if (!r.empty()) check(lvi_marg_add_projection(m_, (int32_t)r.size(), r.data()), "lvi_marg_add_projection");
    }
    void addDense(int32_t rows, const std::vector<int32_t>& ids, const double* residual, const double* jacobians, const std::vector<int32_t>& drop)
    {
        check(lvi_marg_add_dense(m_, rows, (int32_t)ids.size(), ids.data(), residual, jacobians, drop.data()), "lvi_marg_add_dense");
    }
    void addLastPrior(const std::vector<int32_t>& dropIds) { check(lvi_marg_add_last_prior(m_, (int32_t)dropIds.size(), dropIds.data()), "lvi_marg_add_last_prior"); }
    // preMarginalize + marginalize; a soft status is returned, an error thrown
    int32_t marginalize()
    {
        lastStatus = check(lvi_marg_marginalize(m_, &lastInfo), "lvi_marg_marginalize");
        if (lastStatus != LVI_MARG_NOT_FINITE) { valid = true; readLayout(); }
        return lastStatus;
    }
    // getParameterBlocks(addr_shift): the kept ids after the shift
    const std::vector<int32_t>& getParameterBlocks(const std::vector<int32_t>& from, const std::vector<int32_t>& to)
    {
        check(lvi_marg_remap(m_, from.data(), to.data(), (int32_t)from.size()), "lvi_marg_remap");
        readLayout();
        return keepIds;
    }
    bool keeps(int32_t id) const { return valid && std::count(keepIds.begin(), keepIds.end(), id) > 0; }
    // linearized_jacobians [n][n] and linearized_residuals [n]
    void prior(std::vector<double>& J, std::vector<double>& r) const
    {
        const size_t n = (size_t)lastInfo.n;
        J.resize(n * n); r.resize(n);
        check(lvi_marg_get_prior(m_, J.data(), r.data()), "lvi_marg_get_prior");
    }

private:
    void readLayout()
    {
        int32_t k = 0;
        check(lvi_marg_get_layout(m_, nullptr, 0, &k, nullptr, nullptr, nullptr, nullptr), "lvi_marg_get_layout");
        keepIds.resize(k); keepSizes.resize(k); keepIdx.resize(k);
        check(lvi_marg_get_layout(m_, nullptr, k, nullptr, keepIds.data(), keepSizes.data(), keepIdx.data(), nullptr), "lvi_marg_get_layout");
    }
    lvi_marg* m_ = nullptr;
};

// one observation of a feature: FeaturePerFrame's point, velocity, cur_td and uv.y
struct VinsObservation { double point[3], velocity[2], cur_td, uv_y; };
// FeaturePerId: start_frame, feature_per_frame, and its entry of para_Feature
struct VinsFeature { int start_frame = 0; double inv_dep = 0; std::vector<VinsObservation> obs; };

class VinsMarginalizer {
public:
    static constexpr int WINDOW_SIZE = 10;
    enum Flag { MARGIN_OLD = 0, MARGIN_SECOND_NEW = 1 };
    // ids in place of the addresses of para_Pose[k], para_SpeedBias[k], para_Ex_Pose[0], para_Td[0], para_Feature[k]
    static constexpr int32_t ID_POSE = 0, ID_SPEEDBIAS = 16, ID_EX = 32, ID_TD = 33, ID_FEATURE = 64;

    VinsMarginalizer(int device, int max_features, bool estimate_td, const lvi_marg_params* p = nullptr)
        : info(device, caps(max_features), p), estimateTd(estimate_td) {}

    MarginalizationInfo info;
    bool estimateTd;
    double paraPose[WINDOW_SIZE + 1][7] = {}, paraSpeedBias[WINDOW_SIZE + 1][9] = {}, paraExPose[7] = {}, paraTd = 0;
    std::vector<VinsFeature> features;                   // f_manager.feature
    // pre_integrations[1]: sum_dt, and IMUFactor evaluated at (para_Pose[0], para_SpeedBias[0], para_Pose[1], para_SpeedBias[1]):
    // residual [15], jacobians 15x7, 15x9, 15x7, 15x9 in turn.  hasImu false: no factor
    bool hasImu = false;
    double imuSumDt = 0, imuResidual[15] = {}, imuJacobians[15 * 32] = {};

    // estimator.cpp:813-976 -> true when a marginalisation ran
    bool run(Flag flag)
    {
        info.lastStatus = LVI_OK;
        if (flag == MARGIN_OLD) {
            info.begin();
            declareWindow();
            if (info.valid) {                                                        // :818-834
                std::vector<int32_t> drop;
                for (int32_t id : info.keepIds)
                    if (id == ID_POSE || id == ID_SPEEDBIAS) drop.push_back(id);
                info.addLastPrior(drop);
            }
            if (hasImu && imuSumDt < 10.0)                                           // :837-844
                info.addDense(15, {ID_POSE, ID_SPEEDBIAS, ID_POSE + 1, ID_SPEEDBIAS + 1}, imuResidual, imuJacobians, {1, 1, 0, 0});
            std::vector<lvi_marg_projection> recs;                                   // :847-890
            int feature_index = -1;
            for (const VinsFeature& f : features) {
                const int used_num = (int)f.obs.size();
                if (!(used_num >= 2 && f.start_frame < WINDOW_SIZE - 2)) continue;
                ++feature_index;
                const int imu_i = f.start_frame;
                int imu_j = imu_i - 1;
                if (imu_i != 0) continue;
                info.setBlock(ID_FEATURE + feature_index, 1, &f.inv_dep);
                for (const VinsObservation& o : f.obs) {
                    imu_j++;
                    if (imu_i == imu_j) continue;
                    lvi_marg_projection r{};
                    r.pose_i = ID_POSE + imu_i; r.pose_j = ID_POSE + imu_j; r.ex = ID_EX; r.feature = ID_FEATURE + feature_index; r.td = estimateTd ? ID_TD : -1;
                    const VinsObservation& o0 = f.obs[0];
                    for (int k = 0; k < 3; k++) { r.pts_i[k] = o0.point[k]; r.pts_j[k] = o.point[k]; }
                    for (int k = 0; k < 2; k++) { r.velocity_i[k] = o0.velocity[k]; r.velocity_j[k] = o.velocity[k]; }
                    r.td_i = o0.cur_td; r.td_j = o.cur_td; r.row_i = o0.uv_y; r.row_j = o.uv_y;
                    recs.push_back(r);
                }
            }
            info.addProjection(recs);
            if (info.marginalize() == LVI_MARG_NOT_FINITE) return false;
            std::vector<int32_t> from, to;                                           // :896-908
            for (int i = 1; i <= WINDOW_SIZE; i++) { from.push_back(ID_POSE + i); to.push_back(ID_POSE + i - 1); }
            for (int i = 1; i <= WINDOW_SIZE; i++) { from.push_back(ID_SPEEDBIAS + i); to.push_back(ID_SPEEDBIAS + i - 1); }
            info.getParameterBlocks(from, to);
            return true;
        }
        if (!info.keeps(ID_POSE + WINDOW_SIZE - 1)) return false;                    // :918-919
        info.begin();
        declareWindow();
        info.addLastPrior({ID_POSE + WINDOW_SIZE - 1});                              // :926-932
        if (info.marginalize() == LVI_MARG_NOT_FINITE) return false;
        info.getParameterBlocks({ID_POSE + WINDOW_SIZE, ID_SPEEDBIAS + WINDOW_SIZE}, {ID_POSE + WINDOW_SIZE - 1, ID_SPEEDBIAS + WINDOW_SIZE - 1});   // :946-969
        return true;
    }

private:
    static lvi_marg_caps caps(int max_features)
    {
        lvi_marg_caps c;
        c.max_blocks = 2 * (WINDOW_SIZE + 1) + 2 + max_features;
        c.max_projections = std::max(1, max_features * WINDOW_SIZE);
        c.max_dense_factors = 1; c.max_dense_rows = 15;
        c.max_drop_dim = 15 + max_features;
        c.max_keep_dim = 15 * (WINDOW_SIZE + 1) + 7;
        return c;
    }
    // vector2double: every window block at its current value
    void declareWindow()
    {
        for (int k = 0; k <= WINDOW_SIZE; k++) { info.setBlock(ID_POSE + k, 7, paraPose[k]); info.setBlock(ID_SPEEDBIAS + k, 9, paraSpeedBias[k]); }
        info.setBlock(ID_EX, 7, paraExPose);
        info.setBlock(ID_TD, 1, &paraTd);
    }
};

}  // namespace lvi_host
