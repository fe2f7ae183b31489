// C entry points over the loop detector of the host mirror (lvi_bow_host.hpp): LoopDetector::loadVocabulary and
// addKeyFrame, for replay harnesses that are not C++.  include/lvi_bow.h is exported by liblvi_hip.so only, so this file
// is linked into host/liblvi_host_hip.so alone (build.py), never into a host library built against the CPU oracle.
#include "lvi_bow_capi_detail.hpp"
#include "lvi_capi_util.hpp"

using namespace lvi_host;
using lvi_host_capi::Detector;

extern "C" {

const char* lvh_bow_last_error(void) { return g_err.c_str(); }

// a keyframe store (the arguments of lvh_kf_create) with a loop detector of max_entries keyframes over it
void* lvh_bow_create(int32_t device, int32_t max_width, int32_t max_height, int32_t max_keypoints, int32_t max_window, int32_t max_keyframes,
                     const int32_t* x1, const int32_t* y1, const int32_t* x2, const int32_t* y2, int32_t max_entries)
{
    try { return new Detector(max_entries, device, max_width, max_height, max_keypoints, max_window, max_keyframes, x1, y1, x2, y2); }
    catch (const std::exception& e) { g_err = e.what(); return nullptr; }
}

void lvh_bow_destroy(void* d) { delete static_cast<Detector*>(d); }

lvi_kf* lvh_bow_kf_handle(void* d) { return d ? static_cast<Detector*>(d)->kd.get() : nullptr; }
lvi_bow* lvh_bow_db_handle(void* d) { return d ? static_cast<Detector*>(d)->ld.db() : nullptr; }

int32_t lvh_bow_load_vocabulary(void* d, const char* path)
{
    if (!d || !path) return fail("null argument");
    return guarded([&]() -> int32_t { static_cast<Detector*>(d)->ld.loadVocabulary(path); return LVI_OK; });
}

// LoopDetector::addKeyFrame for the keyframe whose device half already lies in `slot` (lvi_kf_describe or lvi_kf_put on
// lvh_bow_kf_handle): the host half is given here, as the loadKeyFrame constructor receives it.  point_3d [n][3],
// point_2d_uv [n][2], point_2d_norm [n][2], point_id [n] (the window); keypoints, keypoints_norm [n_kp][2].
// out[3] = {loop_index, connected, number of query results}; ret = up to 4 result rows (may be NULL).
int32_t lvh_bow_add_keyframe(void* d, int32_t slot, int32_t index, int32_t flag_detect_loop, int32_t n, const float* point_3d, const float* point_2d_uv,
                             const float* point_2d_norm, const double* point_id, int32_t n_kp, const float* keypoints, const float* keypoints_norm,
                             int32_t* out, lvi_bow_result* ret)
{
    if (!d || n < 0 || n_kp < 0 || (n > 0 && (!point_3d || !point_2d_uv || !point_2d_norm || !point_id)) || (n_kp > 0 && (!keypoints || !keypoints_norm)))
        return fail("bad arguments");
    return guarded([&]() -> int32_t {
        Detector* D = static_cast<Detector*>(d);
        KeyFrame kf;
        kf.slot = slot; kf.index = index;
        kf.point_3d.resize(n); kf.point_2d_uv.resize(n); kf.point_2d_norm.resize(n); kf.point_id.assign(point_id, point_id + n);
        for (int i = 0; i < n; i++) {
            kf.point_3d[i] = Point3f{point_3d[3 * i], point_3d[3 * i + 1], point_3d[3 * i + 2]};
            kf.point_2d_uv[i] = Point2f{point_2d_uv[2 * i], point_2d_uv[2 * i + 1]};
            kf.point_2d_norm[i] = Point2f{point_2d_norm[2 * i], point_2d_norm[2 * i + 1]};
        }
        kf.keypoints.resize(n_kp); kf.keypoints_norm.resize(n_kp);
        for (int i = 0; i < n_kp; i++) {
            kf.keypoints[i] = Point2f{keypoints[2 * i], keypoints[2 * i + 1]};
            kf.keypoints_norm[i] = Point2f{keypoints_norm[2 * i], keypoints_norm[2 * i + 1]};
        }
        kf.n_keypoints_found = n_kp;
        D->last = D->ld.addKeyFrame(kf, flag_detect_loop != 0);
        if (out) { out[0] = D->last.loop_index; out[1] = D->last.connected ? 1 : 0; out[2] = (int32_t)D->last.ret.size(); }
        if (ret) for (size_t i = 0; i < D->last.ret.size(); i++) ret[i] = D->last.ret[i];
        return LVI_OK;
    });
}

// the compacted vectors of the last hit's findConnectionFront: cur, old [n][2], id [n] (any may be NULL); returns n
int32_t lvh_bow_connection(void* d, float* cur, float* old_xy, double* id)
{
    if (!d) return fail("null argument");
    const Connection& c = static_cast<Detector*>(d)->last.connection;
    const size_t n = c.matched_2d_cur.size();
    if (cur) for (size_t i = 0; i < n; i++) { cur[2 * i] = c.matched_2d_cur[i].x; cur[2 * i + 1] = c.matched_2d_cur[i].y; }
    if (old_xy) for (size_t i = 0; i < n; i++) { old_xy[2 * i] = c.matched_2d_old[i].x; old_xy[2 * i + 1] = c.matched_2d_old[i].y; }
    if (id) for (size_t i = 0; i < n; i++) id[i] = c.matched_id[i];
    return (int32_t)n;
}

}  // extern "C"
