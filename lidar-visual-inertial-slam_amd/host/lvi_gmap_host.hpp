// Host mirror of mapOptimization's global-map outputs over include/lvi_gmap.h: publishGlobalMap (mapOptimization.cpp
// :460-510), the save_map service (:179-238) and its map files, written as PCL's savePCDFileBinary writes them.
// The key clouds never leave the device but as the fused / filtered result.  Uses the HIP library only (the CPU
// oracle does not export lvi_gmap_*).
#pragma once
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <string>
#include <vector>

#include "../../include/lvi_gmap.h"
#include "lvi_host.hpp"

namespace lvi_host {

// ---- PCD v0.7, DATA binary: the non-padding fields packed, as pcl::io::savePCDFileBinary --------------------------------
inline bool writePCDBinary(const std::string& path, const char* fields, const char* size, const char* type, const char* count,
                           const void* data, size_t n, size_t bytes_per_point)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const std::string hdr = std::string("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS ") + fields + "\nSIZE " + size +
                            "\nTYPE " + type + "\nCOUNT " + count + "\nWIDTH " + std::to_string(n) + "\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS " +
                            std::to_string(n) + "\nDATA binary\n";
    bool ok = std::fwrite(hdr.data(), 1, hdr.size(), f) == hdr.size();
    if (ok && n) ok = std::fwrite(data, bytes_per_point, n, f) == n;
    return std::fclose(f) == 0 && ok;
}
// pcl::PointXYZI: x y z intensity, 16 B per point
inline bool savePCDBinaryXYZI(const std::string& path, const std::vector<lvi_pt>& pts)
{
    return writePCDBinary(path, "x y z intensity", "4 4 4 4", "F F F F", "1 1 1 1", pts.data(), pts.size(), sizeof(lvi_pt));
}
// PointXYZIRPYT (mapOptimization.cpp:29-44): x y z intensity roll pitch yaw as F4, time as F8, 36 B per point
inline bool savePCDBinaryPose6D(const std::string& path, const std::vector<PointTypePose>& poses)
{
    std::vector<unsigned char> buf(poses.size() * 36);
    for (size_t i = 0; i < poses.size(); i++) {
        const PointTypePose& p = poses[i];
        const float f[7] = {p.x, p.y, p.z, p.intensity, p.roll, p.pitch, p.yaw};
        std::memcpy(&buf[i * 36], f, 28);
        std::memcpy(&buf[i * 36 + 28], &p.time, 8);
    }
    return writePCDBinary(path, "x y z intensity roll pitch yaw time", "4 4 4 4 4 4 4 8", "F F F F F F F F", "1 1 1 1 1 1 1 1", buf.data(),
                          poses.size(), 36);
}

struct GlobalMapParams {                        // params_lidar.yaml:82-84
    float globalMapVisualizationSearchRadius = 1000.0f;
    float globalMapVisualizationPoseDensity = 1.0f;
    float globalMapVisualizationLeafSize = 0.05f;
};

class GlobalMapper {
public:
    GlobalMapper(const MapOptimizationNode& node, lvi_lidar* h, const GlobalMapParams& p = GlobalMapParams()) : P(p), node_(node), h_(h) {}
    GlobalMapParams P;

    // the arena of lvi_gmap_build: the node reserves it once at start-up (max_keyframe_points)
    void reserve(int32_t max_points) { check(lvi_gmap_reserve(h_, max_points), "lvi_gmap_reserve"); }

    // publishGlobalMap steps 2-6: the keys whose clouds form globalMapKeyFrames, in fuse order (a key may appear twice)
    std::vector<int32_t> globalMapKeys() const
    {
        const std::vector<lvi_pt>& kp = node_.cloudKeyPoses3D;
        std::vector<int32_t> keys;
        if (kp.empty()) return keys;
        const lvi_pt back = kp.back();
        // radiusSearch (sorted by distance, ties by index), downSizeFilterGlobalMapKeyPoses, nearestKSearch(…, 1)
        std::vector<lvi_pt> ds = downsampleKeyPoses(h_, keyPosesWithin(kp, back, (double)P.globalMapVisualizationSearchRadius),
                                                    P.globalMapVisualizationPoseDensity);
        assignNearestKeys(kp, ds);
        for (const lvi_pt& pt : ds) {
            // pointDistance of the DS centroid (not of the key's own position) to back()
            if (std::sqrt(keyPoseSqDist(pt, back)) > P.globalMapVisualizationSearchRadius) continue;
            keys.push_back((int32_t)pt.intensity);
        }
        return keys;
    }

    // steps 1-6 and the enqueue of step 7: false when there are no key poses.  Returns without waiting for the GPU (the
    // ROS node holds its mutex for this call only).
    bool startGlobalMap()
    {
        if (node_.cloudKeyPoses3D.empty()) return false;
        const std::vector<int32_t> keys = globalMapKeys();
        check(lvi_gmap_build(h_, keys.data(), (int32_t)keys.size(), LVI_GMAP_CORNER_SURF, P.globalMapVisualizationLeafSize, nullptr), "lvi_gmap_build");
        return true;
    }
    // the cloud the reference publishes (PCL's overflow rule: the fused cloud itself); may run beside the scan path
    lvi_gmap_info finishGlobalMap(std::vector<lvi_pt>& out) const
    {
        lvi_gmap_info info{};
        check(lvi_gmap_result(h_, &info), "lvi_gmap_result");
        out.resize(info.n_out);
        check(lvi_gmap_fetch(h_, LVI_GMAP_FILTERED, 0, info.n_out, out.data()), "lvi_gmap_fetch");
        return info;
    }
    bool publishGlobalMap(std::vector<lvi_pt>& out, lvi_gmap_info* info = nullptr)
    {
        if (!startGlobalMap()) return false;
        const lvi_gmap_info r = finishGlobalMap(out);
        if (info) *info = r;
        return true;
    }

    // save_map's fuse (:193-216): all keyframes in index order, corner and surf separately; raw = the fused clouds, ds = the
    // clouds filtered with `resolution` (the raw ones when resolution == 0)
    void fuseAll(float resolution, std::vector<lvi_pt> raw[2], std::vector<lvi_pt> ds[2]) const { fuseAll(resolution, resolution, raw, ds); }
    // … with a leaf of its own per cloud (the shutdown save, :440-452: mappingCornerLeafSize / mappingSurfLeafSize)
    void fuseAll(float leafCorner, float leafSurf, std::vector<lvi_pt> raw[2], std::vector<lvi_pt> ds[2]) const
    {
        std::vector<int32_t> keys(node_.cloudKeyPoses3D.size());
        for (size_t i = 0; i < keys.size(); i++) keys[i] = (int32_t)i;
        for (int w = 0; w < 2; w++) {
            check(lvi_gmap_build(h_, keys.data(), (int32_t)keys.size(), w ? LVI_GMAP_SURF : LVI_GMAP_CORNER, w ? leafSurf : leafCorner, nullptr),
                  "lvi_gmap_build");
            lvi_gmap_info info{};
            check(lvi_gmap_result(h_, &info), "lvi_gmap_result");
            raw[w].resize(info.n_fused); ds[w].resize(info.n_out);
            check(lvi_gmap_fetch(h_, LVI_GMAP_FUSED, 0, info.n_fused, raw[w].data()), "lvi_gmap_fetch");
            check(lvi_gmap_fetch(h_, LVI_GMAP_FILTERED, 0, info.n_out, ds[w].data()), "lvi_gmap_fetch");
        }
    }

    // the save_map service (:179-236): trajectory.pcd, transformations.pcd, CornerMap.pcd, SurfMap.pcd, GlobalMap.pcd in
    // `dir` (created), binary.  Returns what the service's `success` reports: the GlobalMap write.  Deviation: the reference
    // first runs `rm -r` on the directory; here the five files are overwritten and nothing else is touched.
    bool saveMap(const std::string& dir, float resolution) const
    {
        std::error_code ec;
        std::filesystem::create_directories(dir, ec);
        std::vector<lvi_pt> raw[2], ds[2];
        fuseAll(resolution, raw, ds);
        const std::string d = dir.empty() || dir.back() == '/' ? dir : dir + "/";
        savePCDBinaryXYZI(d + "trajectory.pcd", node_.cloudKeyPoses3D);
        savePCDBinaryPose6D(d + "transformations.pcd", node_.cloudKeyPoses6D);
        savePCDBinaryXYZI(d + "CornerMap.pcd", ds[0]);
        savePCDBinaryXYZI(d + "SurfMap.pcd", ds[1]);
        std::vector<lvi_pt> global(raw[0]);
        global.insert(global.end(), raw[1].begin(), raw[1].end());      // the RAW corner cloud, then the RAW surf cloud
        return savePCDBinaryXYZI(d + "GlobalMap.pcd", global);
    }

private:
    const MapOptimizationNode& node_;
    lvi_lidar* h_;
};

}  // namespace lvi_host
