// Host mirror of the visual-inertial alignment of vins_estimator's initialisation over include/lvi_align.h:
//
//   ImageFrames          estimator.cpp:99, :132-135   tmp_pre_integration and the all_image_frame insert
//                        estimator.cpp:1019-1033      the erase of the old slide
//                        estimator.cpp:273-300        the excitation check
//   VisualIMUAlignment   initial_aligment.cpp:201-209 over solveGyroscopeBias, LinearAlignment and RefineGravity
//   visualInitialAlign   estimator.cpp:416-490        over an ImageFrames, an ImuPreintegrator and a FeatureManager
//
// Matrices are row-major.  Header-only, and not included from lvi_host.hpp: only liblvi_hip.so exports this ABI, so only
// code linked against it may include this header.
#pragma once
#include <vector>

#include "../../include/lvi_align.h"
#include "lvi_preint_host.hpp"

namespace lvi_host {

class ImageFrames {
public:
    ImageFrames(int device, int max_frames, int max_samples, const lvi_align_params* p = nullptr)
    {
        const lvi_align_caps caps{max_frames, max_samples};
        check(lvi_align_create(device, &caps, &h_), "lvi_align_create");
        lvi_align_params_default(&params);
        if (p) params = *p;
        if (lvi_align_set_params(h_, &params) < 0) { const Error e(LVI_ERR_INVALID_ARG, "lvi_align_set_params"); lvi_align_destroy(h_); throw e; }
    }
    ~ImageFrames() { lvi_align_destroy(h_); }
    ImageFrames(const ImageFrames&) = delete;
    ImageFrames& operator=(const ImageFrames&) = delete;
    lvi_align* get() const { return h_; }

    lvi_align_params params{};
    lvi_align_info last{};               // of the last VisualIMUAlignment

    void setParameter() { check(lvi_align_set_params(h_, &params), "lvi_align_set_params"); }
    void clearState() { check(lvi_align_clear(h_), "lvi_align_clear"); }
    // :99 for n samples
    void pushIMU(int n, const double* dt, const double* acc, const double* gyr) { check(lvi_align_push_imu(h_, n, dt, acc, gyr), "lvi_align_push_imu"); }
    // :132-135
    void insert(double stamp, const double* Ba, const double* Bg) { check(lvi_align_add_frame(h_, stamp, Ba, Bg), "lvi_align_add_frame"); }
    // :1019-1033
    void eraseThrough(double t_0) { check(lvi_align_erase_through(h_, t_0), "lvi_align_erase_through"); }
    void setPose(double stamp, const double* R, const double* T, bool is_key_frame) { check(lvi_align_set_pose(h_, stamp, R, T, is_key_frame), "lvi_align_set_pose"); }
    int size() const
    {
        int32_t n = 0;
        check(lvi_align_frames(h_, &n), "lvi_align_frames");
        return n;
    }
    lvi_align_frame frame(int index) const
    {
        lvi_align_frame f;
        check(lvi_align_get_frame(h_, index, &f, 0, nullptr, nullptr, nullptr), "lvi_align_get_frame");
        return f;
    }
    // :273-300
    double excitation() const
    {
        double var = 0.;
        check(lvi_align_excitation(h_, &var), "lvi_align_excitation");
        return var;
    }

private:
    lvi_align* h_ = nullptr;
};

// Bgs [11][3] in and out, g [3], x resized to the solution's length.  As in the reference Bgs has been advanced and every
// frame repropagated whatever is returned.
inline bool VisualIMUAlignment(ImageFrames& all_image_frame, double* Bgs, double* g, std::vector<double>& x)
{
    x.assign((size_t)(3 * all_image_frame.size() + 4), 0.);
    check(lvi_align_solve(all_image_frame.get(), Bgs, g, x.data(), (int32_t)x.size(), &all_image_frame.last), "lvi_align_solve");
    x.resize((size_t)all_image_frame.last.n_state);
    return all_image_frame.last.ok != 0;
}

// Estimator::visualInitialAlign.  stamps [frame_count + 1]: Headers[i].stamp of the window's frames.  Ps [11][3], Rs [11][9],
// Vs [11][3], Bgs [11][3], g [3] are the estimator's arrays; ric [9] is RIC[0].  The depth rescale (:467-473), the
// re-triangulation (:437-448) and the window's repropagate (:451-454) stay with the handles that already do them.
inline bool visualInitialAlign(ImageFrames& all_image_frame, ImuPreintegrator& pre_integrations, FeatureManager& f_manager, int frame_count, const double* stamps,
                               double* Ps, double* Rs, double* Vs, double* Bgs, double* g, const double* ric)
{
    std::vector<double> x;
    if (!VisualIMUAlignment(all_image_frame, Bgs, g, x)) return false;
    for (int i = 0; i <= frame_count; i++) {                   // :428-435
        lvi_align_frame f{};
        bool found = false;
        for (int k = 0; k < all_image_frame.size() && !found; k++) {
            f = all_image_frame.frame(k);
            found = f.stamp == stamps[i];
        }
        if (!found) throw Error(LVI_ERR_STATE, "visualInitialAlign: a window frame is not in all_image_frame");
        for (int k = 0; k < 3; k++) Ps[3 * i + k] = f.T[k];
        for (int k = 0; k < 9; k++) Rs[9 * i + k] = f.R[k];
        all_image_frame.setPose(f.stamp, f.R, f.T, true);
    }
    std::vector<double> dep = f_manager.getDepthVector();      // :437-448
    for (double& d : dep) d = -1.;
    f_manager.clearDepth(dep);
    const double tic_tmp[3] = {0., 0., 0.};
    f_manager.triangulate(Ps, Rs, tic_tmp, ric);
    const double zero[33] = {0.};
    pre_integrations.repropagate(zero, Bgs);                   // :451-454
    std::vector<double> key_R;                                 // the kv walk of :457-466
    for (int k = 0; k < all_image_frame.size(); k++) {
        const lvi_align_frame f = all_image_frame.frame(k);
        if (f.is_key_frame) key_R.insert(key_R.end(), f.R, f.R + 9);
    }
    int32_t flags = 0;
    check(lvi_align_apply(&all_image_frame.params, frame_count, Ps, Rs, Vs, x.data(), (int32_t)x.size(), g, key_R.data(), (int32_t)(key_R.size() / 9), nullptr,
                          &flags), "lvi_align_apply");
    dep = f_manager.getDepthVector();                          // :467-473: estimated_depth *= s, as inverse depths
    const double s = x.back();
    for (double& d : dep) d = d / s;
    f_manager.clearDepth(dep);
    return true;
}

}  // namespace lvi_host
