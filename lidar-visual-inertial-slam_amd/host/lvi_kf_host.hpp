// Host-side mirror of the pose_graph KeyFrame over include/lvi_kf.h:
//
//   KeyFrame::KeyFrame (online)     keyframe.cpp:14-34    computeWindowBRIEFPoint + computeBRIEFPoint  -> KeyFrameDescriber::create
//   KeyFrame::findConnection        keyframe.cpp:179-200  searchByBRIEFDes, the six reduceVector compactions and the
//                                                         > MIN_LOOP_NUM gate                           -> KeyFrameDescriber::findConnectionFront
//
// What follows the gate in the reference is PnPRANSAC and the second gate: lvi_pnp_host.hpp's findConnection runs them on
// the device over the compacted vectors left here; the match image stays with the caller.  The DBoW2 query runs on the device over the slot's descriptors (lvi_bow_host.hpp,
// DESIGN §15; the vocabulary file is not shipped, the user supplies it); KeyFrameDescriber::descriptors downloads them for
// savePoseGraph.  Only liblvi_hip.so exports this ABI, so only code linked against it may include this header.  Parity is
// against DESIGN §14's restatement of OpenCV 4.5.x and DVision, not OpenCV itself.
#pragma once
#include <array>
#include <vector>

#include "../../include/lvi_kf.h"
#include "lvi_host.hpp"

namespace lvi_host {

constexpr int MIN_LOOP_NUM = 25;             // keyframe.h:16

// the host half of a KeyFrame: what findConnection reads besides the descriptors (which stay in the device slot)
struct KeyFrame {
    int slot = -1;
    int index = -1;                                       // KeyFrame::index: the LoopDetector's key (lvi_bow_host.hpp)
    std::vector<Point3f> point_3d;
    std::vector<Point2f> point_2d_uv, point_2d_norm;
    std::vector<double> point_id;
    std::vector<Point2f> keypoints, keypoints_norm;       // cv::FAST corners and their MEI lift
    int n_keypoints_found = 0;                            // before the handle's max_keypoints cut
};

// the vectors findConnection holds after the six reduceVector calls: PnPRANSAC's input
struct Connection {
    std::vector<Point2f> matched_2d_cur, matched_2d_old, matched_2d_cur_norm, matched_2d_old_norm;
    std::vector<Point3f> matched_3d;
    std::vector<double> matched_id;
    std::vector<uint8_t> status;                          // searchByBRIEFDes's, before the compaction
    // filled by lvi_pnp_host.hpp's findConnection only: PnPRANSAC's answer, and matched_3d / matched_2d_old_norm as it received them
    std::vector<uint8_t> pnp_status;
    std::vector<Point3f> front_3d;
    std::vector<Point2f> front_2d_old_norm;
};

class KeyFrameDescriber {
public:
    KeyFrameDescriber(int device, int max_width, int max_height, int max_keypoints, int max_window, int max_keyframes, const int32_t* x1,
                      const int32_t* y1, const int32_t* x2, const int32_t* y2)
    {
        check(lvi_kf_create(device, max_width, max_height, max_keypoints, max_window, max_keyframes, x1, y1, x2, y2, &h_), "lvi_kf_create");
    }
    ~KeyFrameDescriber() { lvi_kf_destroy(h_); }
    KeyFrameDescriber(const KeyFrameDescriber&) = delete;
    KeyFrameDescriber& operator=(const KeyFrameDescriber&) = delete;
    lvi_kf* get() const { return h_; }

    // the online KeyFrame constructor: the image work runs on the device into `slot`; the corners come back for
    // findConnection's matched_2d_old
    KeyFrame create(int slot, const uint8_t* img, int w, int h, int stride, const std::vector<Point3f>& point_3d, const std::vector<Point2f>& point_2d_uv,
                    const std::vector<Point2f>& point_2d_norm, const std::vector<double>& point_id, const lvi_mei_params* cam)
    {
        static_assert(sizeof(Point2f) == 2 * sizeof(float), "Point2f must be two packed floats");
        if (point_2d_uv.size() != point_3d.size() || point_2d_uv.size() != point_2d_norm.size() || point_2d_uv.size() != point_id.size())
            throw Error(LVI_ERR_INVALID_ARG, "KeyFrameDescriber::create: the window vectors differ in length");
        KeyFrame kf;
        kf.slot = slot; kf.point_3d = point_3d; kf.point_2d_uv = point_2d_uv; kf.point_2d_norm = point_2d_norm; kf.point_id = point_id;
        lvi_kf_info info{};
        check(lvi_kf_describe(h_, slot, img, w, h, stride, point_2d_uv.empty() ? nullptr : &point_2d_uv[0].x, (int32_t)point_2d_uv.size(), cam, &info),
              "lvi_kf_describe");
        kf.n_keypoints_found = info.n_keypoints_found;
        kf.keypoints.resize(info.n_keypoints_stored);
        kf.keypoints_norm.resize(info.n_keypoints_stored);
        if (info.n_keypoints_stored > 0)
            check(lvi_kf_get(h_, slot, nullptr, &kf.keypoints[0].x, &kf.keypoints_norm[0].x, nullptr, nullptr, nullptr), "lvi_kf_get");
        return kf;
    }

    // brief_descriptors of a slot for savePoseGraph (the DBoW2 query reads them on the device): [n][4] words, bit i of a
    // descriptor in word i >> 6
    std::vector<std::array<uint64_t, 4>> descriptors(int slot)
    {
        int32_t cnt[2] = {0, 0};
        check(lvi_kf_get(h_, slot, cnt, nullptr, nullptr, nullptr, nullptr, nullptr), "lvi_kf_get");
        std::vector<std::array<uint64_t, 4>> d(cnt[0]);
        if (cnt[0] > 0) check(lvi_kf_get(h_, slot, cnt, nullptr, nullptr, d[0].data(), nullptr, nullptr), "lvi_kf_get");
        return d;
    }

    void release(const KeyFrame& kf) { check(lvi_kf_release(h_, kf.slot), "lvi_kf_release"); }

    // findConnection up to PnPRANSAC; true = more than MIN_LOOP_NUM matches survive (the reference goes on to PnPRANSAC)
    bool findConnectionFront(const KeyFrame& cur, const KeyFrame& old_kf, Connection& c)
    {
        const size_t n = cur.point_2d_uv.size();
        c.matched_3d = cur.point_3d;
        c.matched_2d_cur = cur.point_2d_uv;
        c.matched_2d_cur_norm = cur.point_2d_norm;
        c.matched_id = cur.point_id;
        // searchByBRIEFDes
        c.status.assign(n, 0);
        std::vector<int32_t> index(n, -1);
        check(lvi_kf_match(h_, cur.slot, old_kf.slot, c.status.data(), index.data(), nullptr), "lvi_kf_match");
        c.matched_2d_old.assign(n, Point2f{0.f, 0.f});
        c.matched_2d_old_norm.assign(n, Point2f{0.f, 0.f});
        for (size_t i = 0; i < n; i++) {
            if (!c.status[i]) continue;
            c.matched_2d_old[i] = old_kf.keypoints[index[i]];
            c.matched_2d_old_norm[i] = old_kf.keypoints_norm[index[i]];
        }
        reduceVector(c.matched_2d_cur, c.status);
        reduceVector(c.matched_2d_old, c.status);
        reduceVector(c.matched_2d_cur_norm, c.status);
        reduceVector(c.matched_2d_old_norm, c.status);
        reduceVector(c.matched_3d, c.status);
        reduceVector(c.matched_id, c.status);
        return (int)c.matched_2d_cur.size() > MIN_LOOP_NUM;
    }

    template <class T>
    static void reduceVector(std::vector<T>& v, const std::vector<uint8_t>& status)       // keyframe.cpp:3-11
    {
        int j = 0;
        for (int i = 0; i < (int)v.size(); i++)
            if (status[i]) v[j++] = v[i];
        v.resize(j);
    }

private:
    lvi_kf* h_ = nullptr;
};

}  // namespace lvi_host
