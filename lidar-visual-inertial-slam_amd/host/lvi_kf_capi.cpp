// C entry points over the keyframe describer of the host mirror (lvi_kf_host.hpp): the KeyFrame constructor and the front
// half of findConnection, for replay harnesses that are not C++.  include/lvi_kf.h is exported by liblvi_hip.so only, so
// this file is linked into host/liblvi_host_hip.so alone (build.py), never into a host library built against the CPU oracle.
#include <map>

#include "lvi_kf_host.hpp"
#include "lvi_capi_util.hpp"

using namespace lvi_host;

namespace {
struct Matcher {
    KeyFrameDescriber kd;
    std::map<int, KeyFrame> frames;          // by slot
    Connection last;
    template <class... A> explicit Matcher(A... a) : kd(a...) {}
};
}  // namespace

extern "C" {

const char* lvh_kf_last_error(void) { return g_err.c_str(); }

void* lvh_kf_create(int32_t device, int32_t max_width, int32_t max_height, int32_t max_keypoints, int32_t max_window, int32_t max_keyframes,
                    const int32_t* x1, const int32_t* y1, const int32_t* x2, const int32_t* y2)
{
    try { return new Matcher(device, max_width, max_height, max_keypoints, max_window, max_keyframes, x1, y1, x2, y2); }
    catch (const std::exception& e) { g_err = e.what(); return nullptr; }
}

void lvh_kf_destroy(void* m) { delete static_cast<Matcher*>(m); }

lvi_kf* lvh_kf_handle(void* m) { return m ? static_cast<Matcher*>(m)->kd.get() : nullptr; }

// the online KeyFrame constructor into `slot`: point_3d [n][3], point_2d_uv [n][2], point_2d_norm [n][2], point_id [n].
// info[2] = {keypoints found, keypoints stored}
int32_t lvh_kf_add(void* m, int32_t slot, const uint8_t* img, int32_t w, int32_t h, int32_t stride, int32_t n, const float* point_3d,
                   const float* point_2d_uv, const float* point_2d_norm, const double* point_id, const lvi_mei_params* cam, int32_t* info)
{
    if (!m || n < 0 || (n > 0 && (!point_3d || !point_2d_uv || !point_2d_norm || !point_id))) return fail("bad arguments");
    return guarded([&]() -> int32_t {
        Matcher* M = static_cast<Matcher*>(m);
        std::vector<Point3f> p3(n);
        std::vector<Point2f> uv(n), nm(n);
        std::vector<double> id(n);
        for (int i = 0; i < n; i++) {
            p3[i] = Point3f{point_3d[3 * i], point_3d[3 * i + 1], point_3d[3 * i + 2]};
            uv[i] = Point2f{point_2d_uv[2 * i], point_2d_uv[2 * i + 1]};
            nm[i] = Point2f{point_2d_norm[2 * i], point_2d_norm[2 * i + 1]};
            id[i] = point_id[i];
        }
        KeyFrame kf = M->kd.create(slot, img, w, h, stride, p3, uv, nm, id, cam);
        if (info) { info[0] = kf.n_keypoints_found; info[1] = (int32_t)kf.keypoints.size(); }
        M->frames[slot] = std::move(kf);
        return LVI_OK;
    });
}

int32_t lvh_kf_remove(void* m, int32_t slot)
{
    if (!m) return fail("null argument");
    return guarded([&]() -> int32_t {
        Matcher* M = static_cast<Matcher*>(m);
        auto it = M->frames.find(slot);
        if (it == M->frames.end()) return fail("no keyframe in this slot");
        M->kd.release(it->second);
        M->frames.erase(it);
        return LVI_OK;
    });
}

// findConnection up to PnPRANSAC.  Returns 1 when more than MIN_LOOP_NUM matches survive, 0 when not; *n_out = the
// length of the compacted vectors, kept for lvh_kf_connection
int32_t lvh_kf_connect(void* m, int32_t cur_slot, int32_t old_slot, int32_t* n_out)
{
    if (!m) return fail("null argument");
    return guarded([&]() -> int32_t {
        Matcher* M = static_cast<Matcher*>(m);
        auto c = M->frames.find(cur_slot), o = M->frames.find(old_slot);
        if (c == M->frames.end() || o == M->frames.end()) return fail("no keyframe in this slot");
        const bool pass = M->kd.findConnectionFront(c->second, o->second, M->last);
        if (n_out) *n_out = (int32_t)M->last.matched_2d_cur.size();
        return pass ? 1 : 0;
    });
}

// the vectors of the last lvh_kf_connect: cur, old, cur_norm, old_norm [n][2], p3 [n][3], id [n]; status [cap_status]
// = searchByBRIEFDes's (one per window point of cur).  Any pointer may be NULL.
int32_t lvh_kf_connection(void* m, float* cur, float* old_xy, float* cur_norm, float* old_norm, float* p3, double* id, uint8_t* status, int32_t cap_status)
{
    if (!m) return fail("null argument");
    const Connection& c = static_cast<Matcher*>(m)->last;
    const size_t n = c.matched_2d_cur.size();
    auto copy2 = [n](float* dst, const std::vector<Point2f>& v) { if (dst) for (size_t i = 0; i < n; i++) { dst[2 * i] = v[i].x; dst[2 * i + 1] = v[i].y; } };
    copy2(cur, c.matched_2d_cur); copy2(old_xy, c.matched_2d_old); copy2(cur_norm, c.matched_2d_cur_norm); copy2(old_norm, c.matched_2d_old_norm);
    if (p3) for (size_t i = 0; i < n; i++) { p3[3 * i] = c.matched_3d[i].x; p3[3 * i + 1] = c.matched_3d[i].y; p3[3 * i + 2] = c.matched_3d[i].z; }
    if (id) for (size_t i = 0; i < n; i++) id[i] = c.matched_id[i];
    if (status) for (size_t i = 0; i < c.status.size() && (int32_t)i < cap_status; i++) status[i] = c.status[i];
    return (int32_t)n;
}

}  // extern "C"
