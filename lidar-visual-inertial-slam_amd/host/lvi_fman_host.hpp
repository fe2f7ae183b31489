// Host mirror of vins_estimator's FeatureManager over include/lvi_fman.h:
//
//   FeatureManager   feature_manager.{h,cpp}          the reference's method names over the device table
//                    estimator.cpp:639-642             takeDepths: the setDepth half of double2vector
//                    estimator.cpp:1076-1099           slideWindowNew / slideWindowOld with R0, P0, R1, P1 computed as there
//
// fillWindow hands the table to a VinsMarginalizer and a VinsWindowOptimizer, whose `features` and `lidarDepthFlag` the
// caller filled by hand before: add a frame, triangulate, fillWindow, optimize, takeDepths, marginalise, slide,
// removeFailures is the per-image chain of Estimator::processImage.  Only liblvi_hip.so exports this ABI, so only code
// linked against it may include this header.
#pragma once
#include <array>
#include <vector>

#include "../../include/lvi_fman.h"
#include "lvi_win_host.hpp"

namespace lvi_host {

class FeatureManager {
public:
    static constexpr int WINDOW_SIZE = LVI_FMAN_WINDOW;

    FeatureManager(int device, int max_features, const lvi_fman_params* p = nullptr)
    {
        check(lvi_fman_create(device, max_features, &f_), "lvi_fman_create");
        lvi_fman_params_default(&params);
        if (p) params = *p;
        if (lvi_fman_set_params(f_, &params) < 0) { const Error e(LVI_ERR_INVALID_ARG, "lvi_fman_set_params"); lvi_fman_destroy(f_); throw e; }
    }
    ~FeatureManager() { lvi_fman_destroy(f_); }
    FeatureManager(const FeatureManager&) = delete;
    FeatureManager& operator=(const FeatureManager&) = delete;
    lvi_fman* get() const { return f_; }

    lvi_fman_params params{};
    int last_track_num = 0;
    lvi_fman_frame_info lastFrame{};
    lvi_fman_tri_info lastTri{};
    int sum_of_back = 0, sum_of_front = 0;

    void clearState() { check(lvi_fman_clear(f_), "lvi_fman_clear"); }
    int getFeatureCount() const { int32_t n = 0; check(lvi_fman_count(f_, nullptr, &n), "lvi_fman_count"); return n; }
    int size() const { int32_t n = 0; check(lvi_fman_count(f_, &n, nullptr), "lvi_fman_count"); return n; }

    // image: the map of the reference flattened: ids ascending, obs [n][8] = x y z u v vx vy depth
    bool addFeatureCheckParallax(int frame_count, int n, const int32_t* ids, const double* obs, double td)
    {
        check(lvi_fman_add_frame(f_, frame_count, n, ids, obs, td, &lastFrame), "lvi_fman_add_frame");
        last_track_num = lastFrame.last_track_num;
        return lastFrame.keyframe != 0;
    }
    std::vector<std::array<double, 6>> getCorresponding(int frame_count_l, int frame_count_r) const
    {
        std::vector<std::array<double, 6>> out((size_t)size());
        int32_t n = 0;
        check(lvi_fman_corresponding(f_, frame_count_l, frame_count_r, (int32_t)out.size(), &n, out.empty() ? nullptr : out[0].data()), "lvi_fman_corresponding");
        out.resize((size_t)n);
        return out;
    }
    void setDepth(const std::vector<double>& x) { check(lvi_fman_set_depth(f_, (int32_t)x.size(), x.data()), "lvi_fman_set_depth"); }
    void clearDepth(const std::vector<double>& x) { check(lvi_fman_clear_depth(f_, (int32_t)x.size(), x.data()), "lvi_fman_clear_depth"); }
    void removeFailures() { check(lvi_fman_remove_failures(f_), "lvi_fman_remove_failures"); }
    std::vector<double> getDepthVector() const
    {
        std::vector<double> dep((size_t)getFeatureCount());
        if (!dep.empty()) check(lvi_fman_get_depth_vector(f_, (int32_t)dep.size(), nullptr, dep.data()), "lvi_fman_get_depth_vector");
        return dep;
    }
    // Ps [11][3], Rs [11][9] row-major, tic [3], ric [9]
    void triangulate(const double* Ps, const double* Rs, const double* tic, const double* ric)
    {
        check(lvi_fman_triangulate(f_, Ps, Rs, tic, ric, &lastTri), "lvi_fman_triangulate");
    }
    void removeBackShiftDepth(const double* marg_R, const double* marg_P, const double* new_R, const double* new_P)
    {
        check(lvi_fman_remove_back_shift_depth(f_, marg_R, marg_P, new_R, new_P), "lvi_fman_remove_back_shift_depth");
    }
    void removeBack() { check(lvi_fman_remove_back(f_), "lvi_fman_remove_back"); }
    void removeFront(int frame_count) { check(lvi_fman_remove_front(f_, frame_count), "lvi_fman_remove_front"); }
    // `feature`: the list, downloaded
    std::vector<lvi_fman_feature> feature() const
    {
        std::vector<lvi_fman_feature> tab((size_t)size());
        if (!tab.empty()) check(lvi_fman_download(f_, (int32_t)tab.size(), nullptr, tab.data()), "lvi_fman_download");
        return tab;
    }

    // f_manager.feature as the two halves of Estimator::optimization read it: every feature of the table with its
    // start_frame, its observations and the inverse depth getDepthVector gives (vector2double, estimator.cpp:559-562), and
    // lidar_depth_flag beside it
    void fillWindow(VinsMarginalizer& marg, VinsWindowOptimizer& opt) const
    {
        const std::vector<lvi_fman_feature> tab = feature();
        marg.features.assign(tab.size(), VinsFeature());
        opt.lidarDepthFlag.assign(tab.size(), 0);
        for (size_t n = 0; n < tab.size(); n++) {
            const lvi_fman_feature& f = tab[n];
            VinsFeature& v = marg.features[n];
            v.start_frame = f.start_frame;
            v.inv_dep = f.estimated_depth > 0 ? 1. / f.estimated_depth : 1. / params.init_depth;
            v.obs.resize((size_t)f.n_obs);
            for (int k = 0; k < f.n_obs; k++) {
                const lvi_fman_obs& o = f.obs[k];
                VinsObservation& w = v.obs[(size_t)k];
                for (int c = 0; c < 3; c++) w.point[c] = o.point[c];
                for (int c = 0; c < 2; c++) w.velocity[c] = o.velocity[c];
                w.cur_td = o.cur_td; w.uv_y = o.uv[1];
            }
            opt.lidarDepthFlag[n] = f.lidar_depth_flag != 0;
        }
    }
    // double2vector's dep(i) = para_Feature[i][0]; setDepth(dep) (estimator.cpp:639-642): the inverse depths the window solve
    // left in marg.features, which must be the list fillWindow wrote
    void takeDepths(const VinsMarginalizer& marg)
    {
        std::vector<double> dep;
        for (const VinsFeature& v : marg.features)
            if ((int)v.obs.size() >= 2 && v.start_frame < WINDOW_SIZE - 2) dep.push_back(v.inv_dep);
        setDepth(dep);
    }
    // estimator.cpp:1082-1099; back_R0 [9], back_P0 [3]: the oldest frame before the window arrays were shifted; Rs0 [9], Ps0 [3]:
    // frame 0 after it; ric [9], tic [3].  shift_depth: solver_flag == NON_LINEAR
    void slideWindowOld(bool shift_depth, const double* back_R0, const double* back_P0, const double* Rs0, const double* Ps0, const double* ric, const double* tic)
    {
        sum_of_back++;
        if (!shift_depth) { removeBack(); return; }
        double R0[9], R1[9], P0[3], P1[3];
        mul33(back_R0, ric, R0);
        mul33(Rs0, ric, R1);
        mulAdd(back_R0, tic, back_P0, P0);
        mulAdd(Rs0, tic, Ps0, P1);
        removeBackShiftDepth(R0, P0, R1, P1);
    }
    // estimator.cpp:1076-1080
    void slideWindowNew(int frame_count) { sum_of_front++; removeFront(frame_count); }

private:
    // row-major 3 x 3 products, every entry (t0 + t1) + t2 as csrc/lvi_fman_math.hpp and tests/fman_ref.py state them
    static void mul33(const double* A, const double* B, double* C)
    {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
    }
    static void mulAdd(const double* A, const double* x, const double* p, double* y)      // y = p + A x
    {
        for (int i = 0; i < 3; i++) y[i] = p[i] + (A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2]);
    }
    lvi_fman* f_ = nullptr;
};

}  // namespace lvi_host
