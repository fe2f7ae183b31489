// C entry points over the camera rig of the host mirror (lvi_tbatch_host.hpp), for replay harnesses that are not C++.
// include/lvi_tbatch.h is exported by liblvi_hip.so only, so this file is linked into host/liblvi_host_hip.so alone
// (build.py), never into a host library built against the CPU oracle.
//
// One interface, two forms: batched = 1 is FeatureTrackerRig over one lvi_tbatch; batched = 0 is one FeatureTracker over one
// lvi_tracker per camera, called one after another as feature_tracker_node.cpp:136-166 does — the yardstick the rig is held to.
#include <cstring>
#include <memory>

#include "lvi_fmat_host.hpp"
#include "lvi_tbatch_host.hpp"
#include "lvi_capi_util.hpp"

using namespace lvi_host;

struct lvh_rig {
    int S = 0;
    std::unique_ptr<TrackerBatchHandle> b;
    std::unique_ptr<BatchedFundamental> bf;
    std::unique_ptr<FeatureTrackerRig> rig;
    long hook_calls = 0;                                       // findFundamentalMat calls of the per-camera device hooks
    std::vector<std::unique_ptr<TrackerHandle>> th;
    std::vector<std::unique_ptr<FeatureTracker>> ft;
    FeatureTrackerState& cam(int i) { return rig ? rig->trackerData[(size_t)i] : *ft[(size_t)i]; }
};

extern "C" {

const char* lvh_rig_last_error(void) { return g_err.c_str(); }

// cams: [slots] or NULL (no undistortion)
lvh_rig* lvh_rig_create(const lvi_tracker_params* tp, int32_t slots, int32_t device, int32_t row, int32_t col, int32_t equalize, const lvi_mei_params* cams,
                        int32_t batched)
{
    if (!tp || slots < 1 || slots > LVI_TRACKER_MAX_BATCH) { g_err = "bad arguments"; return nullptr; }
    lvh_rig* r = new lvh_rig();
    r->S = slots;
    const int32_t st = guarded([&]() -> int32_t {
        if (batched) {
            r->b.reset(new TrackerBatchHandle(*tp, slots, device));
            r->rig.reset(new FeatureTrackerRig(*r->b, row, col, tp->max_cnt, (int)tp->min_dist));
            if (equalize) r->rig->setEqualize(true);
            if (cams) r->rig->setCameras(cams);
        } else {
            for (int i = 0; i < slots; i++) {
                r->th.emplace_back(new TrackerHandle(*tp, device));
                r->ft.emplace_back(new FeatureTracker(*r->th.back(), row, col, tp->max_cnt, (int)tp->min_dist));
                if (equalize) r->ft.back()->setEqualize(true);
                if (cams) r->ft.back()->setCamera(cams[i]);
            }
        }
        return LVI_OK;
    });
    if (st != LVI_OK) { delete r; return nullptr; }
    return r;
}
void lvh_rig_destroy(lvh_rig* r) { delete r; }

// every camera's findFundamentalMat := a DeviceFundamental of its own (lvi_fmat_host.hpp)
int32_t lvh_rig_use_device_fundamental(lvh_rig* r, int32_t device)
{
    if (!r) return fail("null argument");
    return guarded([&]() -> int32_t {
        for (int i = 0; i < r->S; i++) {
            auto df = std::make_shared<DeviceFundamental>(device);
            r->cam(i).findFundamentalMat = [df, r](const std::vector<Point2f>& a, const std::vector<Point2f>& b, double thr, std::vector<uint8_t>& status) {
                r->hook_calls++;
                df->find(a, b, thr, status);
            };
        }
        return LVI_OK;
    });
}

// rejectWithF of all cameras := ONE BatchedFundamental::find per frame (lvi_fmatb_host.hpp); the batched form only
int32_t lvh_rig_use_batched_fundamental(lvh_rig* r, int32_t device)
{
    if (!r) return fail("null argument");
    if (!r->rig) return fail("the batched rejectWithF needs a rig created with batched = 1", LVI_ERR_STATE);
    return guarded([&]() -> int32_t {
        std::unique_ptr<BatchedFundamental> bf(new BatchedFundamental(device, r->S));
        r->rig->useBatchedFundamental(bf.get());
        r->bf = std::move(bf);
        return LVI_OK;
    });
}

// out[4]: rejectWithF_skipped and rejectWithF_removed summed over the cameras, the findFundamentalMat calls made (batched: the
// handle's calls; otherwise those of the per-camera device hooks), and the cameras that prepared over all frames (batched only)
int32_t lvh_rig_fundamental_stats(lvh_rig* r, int64_t* out)
{
    if (!r || !out) return fail("null argument");
    return guarded([&]() -> int32_t {
        out[0] = out[1] = 0;
        for (int i = 0; i < r->S; i++) { out[0] += r->cam(i).rejectWithF_skipped; out[1] += r->cam(i).rejectWithF_removed; }
        out[2] = r->bf ? r->bf->calls() : r->hook_calls;
        out[3] = r->bf ? r->rig->batchedSlots() : 0;
        return LVI_OK;
    });
}

// imgs[slots] (row x col, tightly packed; NULL = no image for that camera), times[slots], pub_this_frame[slots]
int32_t lvh_rig_read_images(lvh_rig* r, const uint8_t* const* imgs, const double* times, const int32_t* pub_this_frame)
{
    if (!r || !imgs || !times || !pub_this_frame) return fail("null argument");
    return guarded([&]() -> int32_t {
        if (r->rig) {
            bool pub[LVI_TRACKER_MAX_BATCH];
            for (int i = 0; i < r->S; i++) pub[i] = pub_this_frame[i] != 0;
            r->rig->readImages(imgs, times, pub);
        } else {
            for (int i = 0; i < r->S; i++) {
                if (!imgs[i]) continue;
                r->ft[(size_t)i]->PUB_THIS_FRAME = pub_this_frame[i] != 0;
                r->ft[(size_t)i]->readImage(imgs[i], times[i]);
            }
        }
        return LVI_OK;
    });
}

// the node's updateID loop over the cameras (feature_tracker_node.cpp:157-166)
int32_t lvh_rig_update_ids(lvh_rig* r)
{
    if (!r) return fail("null argument");
    for (unsigned int i = 0;; i++) {
        bool completed = false;
        for (int j = 0; j < r->S; j++) completed |= r->cam(j).updateID(i);
        if (!completed) break;
    }
    return LVI_OK;
}
// FeatureTracker::n_id := 0 (the counter is one per process, as the reference's static)
void lvh_rig_reset_ids(void) { FeatureTrackerState::n_id() = 0; }

// one camera's lists after the last frame: xy_un_vel [n][6] = cur_pts, cur_un_pts, pts_velocity; id_cnt [n][2] = ids, track_cnt
int32_t lvh_rig_camera(lvh_rig* r, int32_t cam, float* xy_un_vel, int32_t* id_cnt, int32_t capacity, int32_t* n)
{
    if (!r || !n || cam < 0 || cam >= r->S) return fail("bad argument");
    const FeatureTrackerState& c = r->cam(cam);
    *n = (int32_t)c.cur_pts.size();
    if (!xy_un_vel && !id_cnt) return LVI_OK;
    if (capacity < *n) return fail("capacity too small", LVI_ERR_CAPACITY);
    for (int i = 0; i < *n; i++) {
        const size_t k = (size_t)i;
        if (xy_un_vel) {
            float* row = xy_un_vel + 6 * k;
            row[0] = c.cur_pts[k].x; row[1] = c.cur_pts[k].y;
            row[2] = k < c.cur_un_pts.size() ? c.cur_un_pts[k].x : 0.f; row[3] = k < c.cur_un_pts.size() ? c.cur_un_pts[k].y : 0.f;
            row[4] = k < c.pts_velocity.size() ? c.pts_velocity[k].x : 0.f; row[5] = k < c.pts_velocity.size() ? c.pts_velocity[k].y : 0.f;
        }
        if (id_cnt) { id_cnt[2 * k] = c.ids[k]; id_cnt[2 * k + 1] = c.track_cnt[k]; }
    }
    return LVI_OK;
}

}  // extern "C"
