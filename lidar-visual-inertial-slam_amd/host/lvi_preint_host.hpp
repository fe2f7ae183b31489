// Host mirror of vins_estimator's IMU side over include/lvi_preint.h:
//
//   ImuPreintegrator   estimator.cpp:82-116       processIMU, buffered per image and flushed as one push
//                      integration_base.h:38-52   repropagate of any set of slots in one launch
//                      estimator.cpp:979-1073     the preintegration side of slideWindow's two branches
//                      estimator.cpp:215-269      the lidar branch of initialStructure
//
// fillWindow and fillMarginalizer hand the records to a VinsWindowOptimizer and a VinsMarginalizer through the fields the
// caller filled by hand before (preIntegrations / hasImu; hasImu / imuSumDt / imuResidual / imuJacobians), so
// processIMU ..., flush, fillWindow, optimize, fillMarginalizer, run, setNav, slide is the per-image chain with no
// caller-side IMU arithmetic.  Header-only, and not included from lvi_host.hpp: only liblvi_hip.so exports this ABI, so only
// code linked against it may include this header.
#pragma once
#include <vector>

#include "../../include/lvi_preint.h"
#include "lvi_fman_host.hpp"

namespace lvi_host {

class ImuPreintegrator {
public:
    static constexpr int WINDOW_SIZE = LVI_PREINT_SLOTS - 1;

    ImuPreintegrator(int device, int max_samples, const lvi_preint_params* p = nullptr)
    {
        const lvi_preint_caps caps{max_samples, 0};
        check(lvi_preint_create(device, &caps, &h_), "lvi_preint_create");
        lvi_preint_params_default(&params);
        if (p) params = *p;
        if (lvi_preint_set_params(h_, &params) < 0) { const Error e(LVI_ERR_INVALID_ARG, "lvi_preint_set_params"); lvi_preint_destroy(h_); throw e; }
    }
    ~ImuPreintegrator() { lvi_preint_destroy(h_); }
    ImuPreintegrator(const ImuPreintegrator&) = delete;
    ImuPreintegrator& operator=(const ImuPreintegrator&) = delete;
    lvi_preint* get() const { return h_; }

    lvi_preint_params params{};

    void setParameter() { check(lvi_preint_set_params(h_, &params), "lvi_preint_set_params"); }
    void clearState() { dt_.clear(); acc_.clear(); gyr_.clear(); check(lvi_preint_clear(h_), "lvi_preint_clear"); }

    // processIMU: kept on the host until the image arrives
    void processIMU(double dt, const double* linear_acceleration, const double* angular_velocity)
    {
        dt_.push_back(dt);
        acc_.insert(acc_.end(), linear_acceleration, linear_acceleration + 3);
        gyr_.insert(gyr_.end(), angular_velocity, angular_velocity + 3);
    }
    // the buffered samples as one push with the frame_count they were received under
    void flush(int frame_count)
    {
        check(lvi_preint_push(h_, frame_count, (int32_t)dt_.size(), dt_.data(), acc_.data(), gyr_.data()), "lvi_preint_push");
        dt_.clear(); acc_.clear(); gyr_.clear();
    }
    // Ps, Rs (row-major), Vs, Bas, Bgs of the newest slot: after every solve, before the slide
    void setNav(const double* P, const double* R, const double* V, const double* Ba, const double* Bg)
    {
        lvi_preint_nav n;
        for (int k = 0; k < 3; k++) { n.P[k] = P[k]; n.V[k] = V[k]; n.Ba[k] = Ba[k]; n.Bg[k] = Bg[k]; }
        for (int k = 0; k < 9; k++) n.R[k] = R[k];
        check(lvi_preint_set_nav(h_, &n), "lvi_preint_set_nav");
    }
    lvi_preint_nav nav() const { lvi_preint_nav n; check(lvi_preint_get_nav(h_, &n), "lvi_preint_get_nav"); return n; }
    // Bas [11][3], Bgs [11][3]; mask: bit i for slot i, all eleven by default
    void repropagate(const double* Bas, const double* Bgs, uint32_t mask = (1u << LVI_PREINT_SLOTS) - 1u)
    {
        check(lvi_preint_repropagate(h_, mask, Bas, Bgs), "lvi_preint_repropagate");
    }
    void slideWindowOld() { check(lvi_preint_slide_old(h_), "lvi_preint_slide_old"); }
    void slideWindowNew() { check(lvi_preint_slide_new(h_), "lvi_preint_slide_new"); }
    // the slot's sample count; 0 for a slot that does not exist yet
    int samples(int slot) const
    {
        int32_t n = 0;
        const int32_t st = lvi_preint_get(h_, slot, nullptr, &n);
        if (st == LVI_ERR_STATE) return 0;
        check(st, "lvi_preint_get");
        return n;
    }
    lvi_win_imu record(int slot) const { lvi_win_imu r; check(lvi_preint_get(h_, slot, &r, nullptr), "lvi_preint_get"); return r; }

    // pre_integrations[1..WINDOW_SIZE] of the window solve (estimator.cpp:735-744); a slot without samples, or one that does
    // not exist yet, gives no factor
    void fillWindow(VinsWindowOptimizer& opt) const
    {
        for (int j = 1; j <= WINDOW_SIZE; j++) {
            opt.hasImu[j - 1] = samples(j) > 0;
            if (opt.hasImu[j - 1]) opt.preIntegrations[j - 1] = record(j);
        }
    }
    // the IMU block of MARGIN_OLD (:837-844): pre_integrations[1] evaluated at the marginaliser's blocks 0 and 1
    void fillMarginalizer(VinsMarginalizer& marg) const
    {
        marg.hasImu = samples(1) > 0;
        marg.imuSumDt = 0;
        if (!marg.hasImu) return;
        marg.imuSumDt = record(1).sum_dt;
        check(lvi_preint_evaluate(h_, 1, marg.paraPose[0], marg.paraSpeedBias[0], marg.paraPose[1], marg.paraSpeedBias[1], marg.imuResidual, marg.imuJacobians),
              "lvi_preint_evaluate");
    }
    // The lidar branch of initialStructure (:215-269).  reset_id [11]; T [11][3], R [11][9], Ba, Bg [11][3]: the frames' lidar
    // states; gravity: frame 0's; ric [9] = RIC[0].  false, and nothing changes, when a reset_id is negative or differs from
    // frame 0's; else every slot is repropagated with the frames' biases, params.G becomes (0, 0, gravity) as :253 sets the
    // estimator's g (every later navigation step and lvi_preint_evaluate reads it), every depth is cleared to -1 and the
    // table triangulated with tic = 0.  The caller takes T, R, V, Ba, Bg as its window arrays and params.G as g.
    bool lidarInitialise(FeatureManager& f_manager, const int* reset_id, const double* T, const double* R, const double* Ba, const double* Bg, double gravity,
                         const double* ric)
    {
        for (int i = 0; i <= WINDOW_SIZE; i++)
            if (reset_id[i] < 0 || reset_id[i] != reset_id[0]) return false;
        repropagate(Ba, Bg);
        params.G[0] = 0.; params.G[1] = 0.; params.G[2] = gravity;
        setParameter();
        std::vector<double> dep((size_t)f_manager.getFeatureCount(), -1.0);
        f_manager.clearDepth(dep);
        const double tic[3] = {0., 0., 0.};
        f_manager.triangulate(T, R, tic, ric);
        return true;
    }

private:
    lvi_preint* h_ = nullptr;
    std::vector<double> dt_, acc_, gyr_;
};

}  // namespace lvi_host
