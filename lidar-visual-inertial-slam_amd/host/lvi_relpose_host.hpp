// Host mirror of the first stage of vins_estimator's visual initialisation over include/lvi_relpose.h:
//
//   MotionEstimator    initial/solve_5pts.cpp:193-227   solveRelativeRT on one getCorresponding result
//   relativePose       estimator.cpp:493-522            the frame loop over FeatureManager::getCorresponding
//
// Rotation and Translation are row-major 3 x 3 and 3 doubles.  Header-only, and not included from lvi_host.hpp: only
// liblvi_hip.so exports this ABI, so only code linked against it may include this header.
#pragma once
#include <array>
#include <vector>

#include "../../include/lvi_relpose.h"
#include "lvi_fman_host.hpp"

namespace lvi_host {

class MotionEstimator {
public:
    MotionEstimator(int device, int max_points, int max_iters = 1000, const lvi_relpose_params* p = nullptr)
    {
        check(lvi_relpose_create(device, max_points, max_iters, &h_), "lvi_relpose_create");
        lvi_relpose_params_default(&params);
        if (p) params = *p;
        if (lvi_relpose_set_params(h_, &params) < 0) { const Error e(LVI_ERR_INVALID_ARG, "lvi_relpose_set_params"); lvi_relpose_destroy(h_); throw e; }
    }
    ~MotionEstimator() { lvi_relpose_destroy(h_); }
    MotionEstimator(const MotionEstimator&) = delete;
    MotionEstimator& operator=(const MotionEstimator&) = delete;
    lvi_relpose* get() const { return h_; }

    lvi_relpose_params params{};
    lvi_relpose_result last{};           // of the last solveRelativeRT

    void setParameter() { check(lvi_relpose_set_params(h_, &params), "lvi_relpose_set_params"); }

    // corres: getCorresponding's pairs.  As in the reference Rotation and Translation are written whenever corres.size() >= 15,
    // whatever is returned.
    bool solveRelativeRT(const std::vector<std::array<double, 6>>& corres, double* Rotation, double* Translation)
    {
        check(lvi_relpose_solve(h_, corres.empty() ? nullptr : corres[0].data(), (int32_t)corres.size(), &last, nullptr), "lvi_relpose_solve");
        if (last.flags & LVI_RELPOSE_TOO_FEW) return false;
        for (int k = 0; k < 9; k++) Rotation[k] = last.Rotation[k];
        for (int k = 0; k < 3; k++) Translation[k] = last.Translation[k];
        return last.ok != 0;
    }

private:
    lvi_relpose* h_ = nullptr;
};

// Estimator::relativePose: the first frame of 0 .. WINDOW_SIZE - 1 with more than 20 pairs to the newest frame, an average
// parallax above 30 pixels and a solveRelativeRT that succeeds
inline bool relativePose(const FeatureManager& f_manager, MotionEstimator& m_estimator, double* relative_R, double* relative_T, int& l)
{
    for (int i = 0; i < FeatureManager::WINDOW_SIZE; i++) {
        const std::vector<std::array<double, 6>> corres = f_manager.getCorresponding(i, FeatureManager::WINDOW_SIZE);
        if (corres.size() > 20) {
            const double average_parallax = lvi_relpose_average_parallax(corres[0].data(), (int32_t)corres.size());
            if (average_parallax * 460 > 30 && m_estimator.solveRelativeRT(corres, relative_R, relative_T)) {
                l = i;
                return true;
            }
        }
    }
    return false;
}

}  // namespace lvi_host
