// Host mirror of vins_estimator's window optimisation over include/lvi_win.h:
//
//   WindowProblem         estimator.cpp:698-808   ceres::Problem + ceres::Solve, with ids for addresses
//   VinsWindowOptimizer   estimator.cpp:696-811   the first half of Estimator::optimization over the window arrays a
//                                                 VinsMarginalizer holds, with its id constants
//
// The prior is taken where the marginaliser left it on the device (lvi_win_set_prior_from_marg), so
// `optimize(flag); marginalizer.run(flag);` is the tail of Estimator::optimization with no prior on the bus.  Only
// liblvi_hip.so exports this ABI, so only code linked against it may include this header.
#pragma once
#include <vector>

#include "../../include/lvi_win.h"
#include "lvi_marg_host.hpp"

namespace lvi_host {

class WindowProblem {
public:
    WindowProblem(int device, const lvi_win_caps& caps, const lvi_win_params* p = nullptr)
    {
        check(lvi_win_create(device, &caps, &w_), "lvi_win_create");
        lvi_win_params_default(&params);
        if (p) params = *p;
        if (lvi_win_set_params(w_, &params) < 0) { const Error e(LVI_ERR_INVALID_ARG, "lvi_win_set_params"); lvi_win_destroy(w_); throw e; }
    }
    ~WindowProblem() { lvi_win_destroy(w_); }
    WindowProblem(const WindowProblem&) = delete;
    WindowProblem& operator=(const WindowProblem&) = delete;
    lvi_win* get() const { return w_; }

    lvi_win_params params{};
    lvi_win_info lastInfo{};
    int32_t lastStatus = LVI_OK;

    void setParams() { check(lvi_win_set_params(w_, &params), "lvi_win_set_params"); }
    void begin() { check(lvi_win_begin(w_), "lvi_win_begin"); }
    void addParameterBlock(int32_t id, int32_t size, const double* v, int32_t flags = 0) { check(lvi_win_set_block(w_, id, size, v, flags), "lvi_win_set_block"); }
    void addProjection(const std::vector<lvi_marg_projection>& r)
    {
        if (!r.empty()) check(lvi_win_add_projection(w_, (int32_t)r.size(), r.data()), "lvi_win_add_projection");
    }
    void addImu(const lvi_win_imu& r) { check(lvi_win_add_imu(w_, 1, &r), "lvi_win_add_imu"); }
    void setPrior(const MarginalizationInfo& m) { check(lvi_win_set_prior_from_marg(w_, m.get()), "lvi_win_set_prior_from_marg"); }
    // ceres::Solve; a soft status is returned, an error thrown
    int32_t solve() { return lastStatus = check(lvi_win_solve(w_, &lastInfo), "lvi_win_solve"); }
    void block(int32_t id, double* v) const { check(lvi_win_get_block(w_, id, v), "lvi_win_get_block"); }
    std::vector<lvi_win_iteration> log() const
    {
        int32_t n = 0;
        check(lvi_win_get_log(w_, 0, &n, nullptr), "lvi_win_get_log");
        std::vector<lvi_win_iteration> out((size_t)n);
        if (n > 0) check(lvi_win_get_log(w_, n, nullptr, out.data()), "lvi_win_get_log");
        return out;
    }

private:
    lvi_win* w_ = nullptr;
};

class VinsWindowOptimizer {
public:
    static constexpr int WINDOW_SIZE = VinsMarginalizer::WINDOW_SIZE;

    // window: the marginaliser whose arrays (paraPose, paraSpeedBias, paraExPose, paraTd, features) are optimised in place
    VinsWindowOptimizer(VinsMarginalizer& window, int device, int max_features, const lvi_win_params* p = nullptr)
        : win(window), problem(device, caps(max_features), p) {}

    VinsMarginalizer& win;
    WindowProblem problem;
    int estimateExtrinsic = 0;                           // ESTIMATE_EXTRINSIC: 0 holds para_Ex_Pose constant (:712-716)
    int numIterations = 8;                               // NUM_ITERATIONS
    double solverTime = 0.;                              // SOLVER_TIME in seconds; 0: no limit
    std::vector<char> lidarDepthFlag;                    // per entry of win.features: lidar_depth_flag (:775, :784); missing entries are false
    // pre_integrations[j], j = 1..WINDOW_SIZE at index j - 1: the ids are filled in here; hasImu false or sum_dt > 10 (:740): no factor
    lvi_win_imu preIntegrations[WINDOW_SIZE] = {};
    bool hasImu[WINDOW_SIZE] = {};

    // estimator.cpp:696-811 -> the solve's status; the window arrays and the features' inverse depths hold the result
    int32_t optimize(VinsMarginalizer::Flag flag)
    {
        using V = VinsMarginalizer;
        problem.begin();
        for (int i = 0; i <= WINDOW_SIZE; i++) {                                       // :702-707
            problem.addParameterBlock(V::ID_POSE + i, 7, win.paraPose[i]);
            problem.addParameterBlock(V::ID_SPEEDBIAS + i, 9, win.paraSpeedBias[i]);
        }
        problem.addParameterBlock(V::ID_EX, 7, win.paraExPose, estimateExtrinsic ? 0 : LVI_WIN_CONSTANT);      // :708-719
        if (win.estimateTd) problem.addParameterBlock(V::ID_TD, 1, &win.paraTd);         // :720-724
        std::vector<lvi_marg_projection> recs;                                         // :745-789
        std::vector<int> featureOf;
        int feature_index = -1;
        for (size_t n = 0; n < win.features.size(); n++) {
            const VinsFeature& f = win.features[n];
            const int used_num = (int)f.obs.size();
            if (!(used_num >= 2 && f.start_frame < WINDOW_SIZE - 2)) continue;
            ++feature_index;
            const int imu_i = f.start_frame;
            int imu_j = imu_i - 1;
            const bool lidar = n < lidarDepthFlag.size() && lidarDepthFlag[n];
            problem.addParameterBlock(V::ID_FEATURE + feature_index, 1, &f.inv_dep, lidar ? LVI_WIN_CONSTANT : LVI_WIN_ELIMINATED);
            featureOf.push_back((int)n);
            for (const VinsObservation& o : f.obs) {
                imu_j++;
                if (imu_i == imu_j) continue;
                lvi_marg_projection r{};
                r.pose_i = V::ID_POSE + imu_i; r.pose_j = V::ID_POSE + imu_j; r.ex = V::ID_EX; r.feature = V::ID_FEATURE + feature_index;
                r.td = win.estimateTd ? V::ID_TD : -1;
                const VinsObservation& o0 = f.obs[0];
                for (int k = 0; k < 3; k++) { r.pts_i[k] = o0.point[k]; r.pts_j[k] = o.point[k]; }
                for (int k = 0; k < 2; k++) { r.velocity_i[k] = o0.velocity[k]; r.velocity_j[k] = o.velocity[k]; }
                r.td_i = o0.cur_td; r.td_j = o.cur_td; r.row_i = o0.uv_y; r.row_j = o.uv_y;
                recs.push_back(r);
            }
        }
        problem.addProjection(recs);
        for (int i = 0; i < WINDOW_SIZE; i++) {                                        // :737-744
            if (!hasImu[i] || preIntegrations[i].sum_dt > 10.0) continue;
            lvi_win_imu r = preIntegrations[i];
            r.pose_i = V::ID_POSE + i; r.speed_bias_i = V::ID_SPEEDBIAS + i; r.pose_j = V::ID_POSE + i + 1; r.speed_bias_j = V::ID_SPEEDBIAS + i + 1;
            problem.addImu(r);
        }
        if (win.info.valid) problem.setPrior(win.info);                                // :729-735
        problem.params.max_iterations = numIterations;                                 // :798-805
        problem.params.max_time_s = flag == V::MARGIN_OLD ? solverTime * 4.0 / 5.0 : solverTime;
        problem.setParams();
        const int32_t st = problem.solve();                                            // :808
        if (st != LVI_OK) return st;
        for (int i = 0; i <= WINDOW_SIZE; i++) {                                       // :811, what double2vector reads
            problem.block(V::ID_POSE + i, win.paraPose[i]);
            problem.block(V::ID_SPEEDBIAS + i, win.paraSpeedBias[i]);
        }
        problem.block(V::ID_EX, win.paraExPose);
        if (win.estimateTd) problem.block(V::ID_TD, &win.paraTd);
        for (size_t k = 0; k < featureOf.size(); k++) problem.block(V::ID_FEATURE + (int)k, &win.features[featureOf[k]].inv_dep);
        return st;
    }

private:
    static lvi_win_caps caps(int max_features)
    {
        lvi_win_caps c;
        c.max_blocks = 2 * (WINDOW_SIZE + 1) + 2 + max_features;
        c.max_projections = std::max(1, max_features * WINDOW_SIZE);
        c.max_eliminated = max_features;
        c.max_imu = WINDOW_SIZE;
        c.max_prior_rows = 15 * (WINDOW_SIZE + 1) + 7;
        c.max_dim = 15 * (WINDOW_SIZE + 1) + 7;
        return c;
    }
};

}  // namespace lvi_host
