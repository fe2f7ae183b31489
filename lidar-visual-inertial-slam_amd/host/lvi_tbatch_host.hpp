// Host-side mirror for camera rigs: S FeatureTracker states over ONE batch tracker handle (include/lvi_tbatch.h), so that a frame
// of S cameras costs the launch chain and the two waits of one camera.
//
//   feature_tracker_node.cpp:136-166   for (i < NUM_OF_CAM) trackerData[i].readImage(...);  then the updateID loop
//
// The reference compiles NUM_OF_CAM = 1 (parameters.h), so its loop runs once: this class is a capability of the library for
// rigs, several robots on one device or sharded replay, not a restated reference behaviour.  Every camera's lists equal those
// of a FeatureTracker (host/lvi_host.hpp) given the same images, times and PUB_THIS_FRAME: both run FeatureTrackerState's code
// around their device calls.  include/lvi_tbatch.h is exported by liblvi_hip.so only.
#pragma once
#include <memory>

#include "../../include/lvi_tbatch.h"
#include "lvi_fmatb_host.hpp"
#include "lvi_host.hpp"

namespace lvi_host {

class TrackerBatchHandle {
public:
    TrackerBatchHandle(const lvi_tracker_params& p, int slots, int device) : P(p), slots(slots) { check(lvi_tbatch_create(&p, slots, device, &b_), "lvi_tbatch_create"); }
    ~TrackerBatchHandle() { lvi_tbatch_destroy(b_); }
    TrackerBatchHandle(const TrackerBatchHandle&) = delete;
    TrackerBatchHandle& operator=(const TrackerBatchHandle&) = delete;
    lvi_tbatch* get() const { return b_; }
    lvi_tracker_params P;
    int slots;
private:
    lvi_tbatch* b_ = nullptr;
};

class FeatureTrackerRig {
public:
    FeatureTrackerRig(TrackerBatchHandle& b, int row, int col, int max_cnt, int min_dist)
        : trackerData((size_t)b.slots, FeatureTrackerState(row, col, max_cnt, min_dist)), b_(b), S(b.slots), ROW(row), COL(col), MIN_DIST(min_dist) {}

    std::vector<FeatureTrackerState> trackerData;              // [NUM_OF_CAM]

    // EQUALIZE (feature_tracker.cpp:86-90) for every camera
    void setEqualize(bool on) { check(lvi_tbatch_set_equalize(b_.get(), on ? 1 : 0, 3.0, 8, 8), "lvi_tbatch_set_equalize"); }
    // one MEI model per camera; all cameras or none
    void setCameras(const lvi_mei_params* cams)
    {
        cams_.assign(cams, cams + S);
        for (int i = 0; i < S; i++) trackerData[(size_t)i].setCamera(cams[i]);
    }

    // FeatureTracker::readImage for every camera (imgs[i] == nullptr: camera i has no image this frame and keeps its state), in
    // three phases around the handle's two waits
    void readImages(const uint8_t* const* imgs, const double* times, const bool* pub_this_frame)
    {
        const size_t F = (size_t)b_.P.max_features;
        const bool want_un = !cams_.empty();
        std::vector<const float*> ptr((size_t)S, nullptr);
        std::vector<int32_t> n((size_t)S, -1);
        // ---- 1: push, set_points and run_lk for all cameras, ONE wait
        bool any_lk = false;
        for (int i = 0; i < S; i++) {
            if (!imgs[i]) continue;
            FeatureTrackerState& c = trackerData[(size_t)i];
            c.cur_time = times[i]; c.PUB_THIS_FRAME = pub_this_frame[i];
            c.forw_pts.clear();
            if (!c.cur_pts.empty()) { ptr[(size_t)i] = &c.cur_pts[0].x; n[(size_t)i] = (int32_t)c.cur_pts.size(); any_lk = true; }
        }
        check(lvi_tbatch_push_images(b_.get(), imgs, COL, ROW, COL), "lvi_tbatch_push_images");   // forw_img = img (:94-101)
        if (any_lk) {
            check(lvi_tbatch_set_points(b_.get(), ptr.data(), n.data()), "lvi_tbatch_set_points");
            check(lvi_tbatch_run_lk(b_.get()), "lvi_tbatch_run_lk");                               // calcOpticalFlowPyrLK (:113)
        }
        // ---- 2: per camera the border test, reduceVector, rejectWithF through its hook, setMask's walk; circles and GFTT for all
        //         (with useBatchedFundamental: rejectWithF for all cameras in ONE call between its two halves)
        std::vector<int32_t> quota((size_t)S, -1), n_kept((size_t)S, -1);
        bool any_gftt = false, any_end = false;
        auto lkResults = [&](int i) {
            const int32_t n_lk = n[(size_t)i];
            if (n_lk <= 0) return;
            FeatureTrackerState& c = trackerData[(size_t)i];
            std::vector<uint8_t> status((size_t)n_lk);
            std::vector<float> err((size_t)n_lk);
            c.forw_pts.resize((size_t)n_lk);
            int32_t m = 0;
            check(lvi_tbatch_get_lk(b_.get(), i, &c.forw_pts[0].x, status.data(), err.data(), n_lk, &m), "lvi_tbatch_get_lk");
            c.applyLkStatus(status);
        };
        if (bf_) {
            const std::vector<Point2f>* none = nullptr;
            std::vector<const std::vector<Point2f>*> pa((size_t)S, none), pb((size_t)S, none);
            std::vector<double> thr((size_t)S, 0.0);
            bool any_prepared = false;
            un_a_.resize((size_t)S); un_b_.resize((size_t)S);
            for (int i = 0; i < S; i++) {
                if (!imgs[i]) continue;
                FeatureTrackerState& c = trackerData[(size_t)i];
                lkResults(i);
                c.bumpTrackCnt();
                if (c.PUB_THIS_FRAME && c.prepareRejectWithF(un_a_[(size_t)i], un_b_[(size_t)i])) {
                    pa[(size_t)i] = &un_a_[(size_t)i]; pb[(size_t)i] = &un_b_[(size_t)i]; thr[(size_t)i] = c.F_THRESHOLD;
                    any_prepared = true; batched_slots_++;
                }
            }
            if (any_prepared) {
                bf_->find(pa, pb, thr, f_status_);
                for (int i = 0; i < S; i++) if (pa[(size_t)i]) trackerData[(size_t)i].applyRejectWithF(f_status_[(size_t)i]);
            }
        }
        for (int i = 0; i < S; i++) {
            ptr[(size_t)i] = nullptr;
            if (!bf_ && imgs[i]) lkResults(i);
            n[(size_t)i] = -1;
            if (!imgs[i]) continue;
            FeatureTrackerState& c = trackerData[(size_t)i];
            const int n_max_cnt = !bf_ ? c.beginDetection() : c.PUB_THIS_FRAME ? c.maskAndQuota() : 0;
            if (n_max_cnt > 0) {
                ptr[(size_t)i] = c.forw_pts.empty() ? nullptr : &c.forw_pts[0].x; n[(size_t)i] = (int32_t)c.forw_pts.size();
                quota[(size_t)i] = n_max_cnt; any_gftt = true;
            }
            if (n_max_cnt > 0 || (want_un && !c.forw_pts.empty())) { n_kept[(size_t)i] = (int32_t)c.forw_pts.size(); any_end = true; }
        }
        if (any_gftt) {
            check(lvi_tbatch_set_mask_circles(b_.get(), ptr.data(), n.data(), MIN_DIST), "lvi_tbatch_set_mask_circles");
            check(lvi_tbatch_run_gftt_async(b_.get(), quota.data()), "lvi_tbatch_run_gftt_async");   // goodFeaturesToTrack (:166)
        }
        // ---- the ONE read that ends the frame for all cameras
        if (out_.size() != (size_t)S * F) { out_.assign((size_t)S * F, Point2f{0.f, 0.f}); un_.assign((size_t)S * F, Point2f{0.f, 0.f}); }
        std::vector<float*> new_p((size_t)S), un_p((size_t)S);
        std::vector<int32_t> n_new((size_t)S, 0);
        for (int i = 0; i < S; i++) {
            FeatureTrackerState& c = trackerData[(size_t)i];
            ptr[(size_t)i] = (n_kept[(size_t)i] > 0) ? &c.forw_pts[0].x : nullptr;
            new_p[(size_t)i] = &out_[(size_t)i * F].x; un_p[(size_t)i] = &un_[(size_t)i * F].x;
        }
        if (any_end)
            check(lvi_tbatch_finish_frame(b_.get(), want_un ? cams_.data() : nullptr, ptr.data(), n_kept.data(), new_p.data(), (int32_t)F, n_new.data(),
                                          want_un ? un_p.data() : nullptr), "lvi_tbatch_finish_frame");
        // ---- 3: per camera addPoints, the rotation and undistortedPoints
        for (int i = 0; i < S; i++) {
            if (!imgs[i]) continue;
            FeatureTrackerState& c = trackerData[(size_t)i];
            c.endFrame(&out_[(size_t)i * F], quota[(size_t)i] > 0 ? n_new[(size_t)i] : 0, want_un ? &un_[(size_t)i * F] : nullptr);
            if (want_un) {                                                                        // :205
                if (!c.takeReadyUndistorted()) throw std::logic_error("FeatureTrackerRig: the frame end did not return the undistorted points");
                c.velocityMap();
            }
            c.prev_time = c.cur_time;
        }
    }
    // the node's loop over the cameras, feature_tracker_node.cpp:157-166 (STEREO_TRACK off)
    void updateIDs()
    {
        for (unsigned int i = 0;; i++) {
            bool completed = false;
            for (int j = 0; j < S; j++) completed |= trackerData[(size_t)j].updateID(i);
            if (!completed) break;
        }
    }
    // rejectWithF of all cameras := one BatchedFundamental::find per frame (host/lvi_fmatb_host.hpp) between prepareRejectWithF and
    // applyRejectWithF; the cameras' own findFundamentalMat hooks are then not called.  nullptr: the per-camera hooks again.
    void useBatchedFundamental(BatchedFundamental* bf)
    {
        if (bf && bf->slots() != S) throw Error(LVI_ERR_INVALID_ARG, "FeatureTrackerRig::useBatchedFundamental: one slot per camera");
        bf_ = bf;
    }
    long batchedSlots() const { return batched_slots_; }       // cameras that prepared, over all frames: the calls per-camera hooks would have made
private:
    TrackerBatchHandle& b_;
    int S, ROW, COL, MIN_DIST;
    std::vector<lvi_mei_params> cams_;
    std::vector<Point2f> out_, un_;
    BatchedFundamental* bf_ = nullptr;
    long batched_slots_ = 0;
    std::vector<std::vector<Point2f>> un_a_, un_b_;            // un_cur_pts, un_forw_pts per camera
    std::vector<std::vector<uint8_t>> f_status_;
};

}  // namespace lvi_host
