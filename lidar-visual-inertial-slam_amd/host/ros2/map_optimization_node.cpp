// Drop-in for the scan-matching half of lidar_odometry/src/mapOptimization.cpp: same node name, topics, QoS, frame ids and
// odometry messages (mapOptimization.cpp:161-177, 238-245, 298-333, 1666-1746).  updateInitialGuess, extractNearby, the
// keyframe decision and the key poses run in lvi_host::MapOptimizationNode (host C++ over the C-ABI); the keyframe clouds,
// the local map (incremental lvi_map_update), downsampleCurrentScan and scan2MapOptimization run on the MI355X.
// The global map (publishGlobalMap on its 0.2 Hz thread, :421-427 / :460-510), the save_map service (:179-238) and the
// shutdown save (:428-457) fuse the device keyframe store on the MI355X through lvi_host::GlobalMapper (include/lvi_gmap.h);
// the files are written with pcl::io as the reference writes them.  Deviation: the directory is created and the files are
// overwritten; the reference's `rm -r` of the directory is not reproduced.
// The loop-closure thread (:523-535) runs performLoopClosure through lvi_host::LoopCloser (include/lvi_loop.h): the key
// search on the host, the two submaps and the ICP on the MI355X; it publishes the two clouds and visualizeLoopClosure's
// markers and leaves the constraints in takeLoopConstraints().
// With the parameter use_device_pose_graph (default false) the node applies them: addOdomFactor, addLoopFactor, the
// updates and correctPoses (:1414-1428, 1509-1527, 1546-1599, 1615-1646) run through lvi_host::PoseGraphBackend
// (include/lvi_pgo.h: the minimiser of the graph's cost on the MI355X, not iSAM2's iterate), and the path is rebuilt after
// a correction (:1641-1645).  Without it the key pose pushed is the scan-matching result ("odometry chain"), which does not
// consume the constraint queue.  With the pose graph the node also subscribes to gpsTopic (:172-174): gpsHandler (:334-337)
// forwards each message to lvi_host::MapOptimizationNode::gpsHandler, whose GpsGate (host/lvi_gps_gate.hpp) restates
// addGPSFactor (:1430-1507) over include/lvi_pgo_gps.h with useGpsElevation, gpsCovThreshold and poseCovThreshold.
// Builds only where rclcpp, tf2_ros, pcl_conversions and the lidar_odometry messages / services exist.
#include <cstdlib>
#include <deque>
#include <iostream>
#include <filesystem>
#include <mutex>
#include <thread>

#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <pcl_conversions/pcl_conversions.h>
#include <rclcpp/rclcpp.hpp>
#include <nav_msgs/msg/odometry.hpp>
#include <nav_msgs/msg/path.hpp>
#include <sensor_msgs/msg/point_cloud2.hpp>
#include <std_msgs/msg/float64_multi_array.hpp>
#include <visualization_msgs/msg/marker_array.hpp>
#include <tf2/LinearMath/Quaternion.h>
#include <tf2_geometry_msgs/tf2_geometry_msgs.hpp>
#include <tf2_ros/transform_broadcaster.h>

#include "../lvi_gmap_host.hpp"
#include "../lvi_host.hpp"
#include "../lvi_loop_host.hpp"
#include "../lvi_pgo_host.hpp"
#include "lidar_odometry/msg/cloud_info.hpp"
#include "lidar_odometry/srv/save_map.hpp"
#include "utility.h"   // the reference's ParamServer, publishCloud, qos, stamp2Sec (and pcl/io/pcd_io.h)

// cloudKeyPoses6D's point type (mapOptimization.cpp:29-44): x y z intensity roll pitch yaw (float), time (double)
struct PointXYZIRPYT {
    PCL_ADD_POINT4D;
    PCL_ADD_INTENSITY;
    float roll;
    float pitch;
    float yaw;
    double time;
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
} EIGEN_ALIGN16;
POINT_CLOUD_REGISTER_POINT_STRUCT(PointXYZIRPYT, (float, x, x)(float, y, y)(float, z, z)(float, intensity, intensity)(float, roll, roll)
                                                 (float, pitch, pitch)(float, yaw, yaw)(double, time, time))

class mapOptimization : public ParamServer {
    rclcpp::Publisher<nav_msgs::msg::Odometry>::SharedPtr pubLaserOdometryGlobal, pubLaserOdometryIncremental;
    rclcpp::Publisher<sensor_msgs::msg::PointCloud2>::SharedPtr pubKeyPoses, pubRecentKeyFrames, pubLaserCloudSurround;
    rclcpp::Publisher<nav_msgs::msg::Path>::SharedPtr pubPath;
    rclcpp::Publisher<sensor_msgs::msg::PointCloud2>::SharedPtr pubHistoryKeyFrames, pubIcpKeyFrames;
    rclcpp::Publisher<visualization_msgs::msg::MarkerArray>::SharedPtr pubLoopConstraintEdge;
    rclcpp::Subscription<std_msgs::msg::Float64MultiArray>::SharedPtr subLoop;
    rclcpp::Subscription<lidar_odometry::msg::CloudInfo>::SharedPtr subCloud;
    rclcpp::Subscription<nav_msgs::msg::Odometry>::SharedPtr subGPS;
    rclcpp::Service<lidar_odometry::srv::SaveMap>::SharedPtr srvSaveMap;
    std::unique_ptr<tf2_ros::TransformBroadcaster> br;
    std::mutex mtx;               // the node's state and every call on the handle but lvi_gmap_result / lvi_gmap_fetch / lvi_loop_result / lvi_loop_fetch
    std::mutex gmapMtx;           // one global-map build at a time, with its result / fetch (taken before mtx)
    std::unique_ptr<lvi_host::LidarHandle> handle;
    std::unique_ptr<lvi_host::MapOptimizationNode> mo;
    std::unique_ptr<lvi_host::GlobalMapper> gmap;
    std::mutex loopMtx;           // one loop job at a time, with its result / fetch (taken before mtx)
    std::mutex mtxLoopInfo;       // loopInfoVec (:539)
    std::mutex loopQueueMtx;      // the constraint queue
    std::unique_ptr<lvi_host::LoopCloser> loop;
    std::deque<lvi_host::LoopConstraint> loopConstraints;      // loopIndexQueue / loopPoseQueue / loopNoiseQueue
    std::unique_ptr<lvi_host::PoseGraphBackend> poseGraph;     // use_device_pose_graph
    int posesCorrectedSeen = 0;
    rclcpp::Time timeLaserInfoStamp;
    nav_msgs::msg::Path globalPath;
    // incremental odometry (publishOdometry :1693-1741)
    bool lastIncreOdomPubFlag = false;
    nav_msgs::msg::Odometry laserOdomIncremental;
    lvi_host::Affine3f increOdomAffine{}, incrementalOdometryAffineFront{};

public:
    explicit mapOptimization(const rclcpp::NodeOptions& options) : ParamServer("mapOptimization", options)
    {
        lvi_lidar_params p; lvi_lidar_params_default(&p);
        p.N_SCAN = N_SCAN; p.Horizon_SCAN = Horizon_SCAN;
        p.edgeFeatureMinValidNum = edgeFeatureMinValidNum; p.surfFeatureMinValidNum = surfFeatureMinValidNum;
        p.mappingCornerLeafSize = mappingCornerLeafSize; p.mappingSurfLeafSize = mappingSurfLeafSize;
        p.z_tollerance = z_tollerance; p.rotation_tollerance = rotation_tollerance; p.imuRPYWeight = imuRPYWeight;
        p.max_raw_points = N_SCAN * Horizon_SCAN; p.max_map_points = 1 << 23; p.max_keyframes = 8192; p.max_keyframe_points = 1 << 25;
        handle = std::make_unique<lvi_host::LidarHandle>(p, 0);
        lvi_host::MapCallerParams c;
        c.useImuHeadingInitialization = useImuHeadingInitialization; c.mappingProcessInterval = mappingProcessInterval;
        c.surroundingkeyframeAddingDistThreshold = surroundingkeyframeAddingDistThreshold;
        c.surroundingkeyframeAddingAngleThreshold = surroundingkeyframeAddingAngleThreshold;
        c.surroundingKeyframeDensity = surroundingKeyframeDensity; c.surroundingKeyframeSearchRadius = surroundingKeyframeSearchRadius;
        c.sensorIsLivox = sensor == SensorType::LIVOX;
        mo = std::make_unique<lvi_host::MapOptimizationNode>(*handle, c);
        lvi_host::GlobalMapParams g;
        g.globalMapVisualizationSearchRadius = globalMapVisualizationSearchRadius;
        g.globalMapVisualizationPoseDensity = globalMapVisualizationPoseDensity;
        g.globalMapVisualizationLeafSize = globalMapVisualizationLeafSize;
        gmap = std::make_unique<lvi_host::GlobalMapper>(*mo, handle->get(), g);
        gmap->reserve(p.max_keyframe_points);                                                                          // the arena, once
        lvi_host::LoopParams lpp;
        lpp.loopClosureEnableFlag = loopClosureEnableFlag; lpp.loopClosureFrequency = loopClosureFrequency;
        lpp.historyKeyframeSearchRadius = historyKeyframeSearchRadius; lpp.historyKeyframeSearchTimeDiff = historyKeyframeSearchTimeDiff;
        lpp.historyKeyframeSearchNum = historyKeyframeSearchNum; lpp.historyKeyframeFitnessScore = historyKeyframeFitnessScore;
        lpp.mappingSurfLeafSize = mappingSurfLeafSize;
        loop = std::make_unique<lvi_host::LoopCloser>(*mo, handle->get(), lpp);
        if (loopClosureEnableFlag) loop->reserve(1 << 20, 1 << 24);                                                    // the arena, once: one key / 2 n + 1 keys
        if (declare_parameter<bool>("use_device_pose_graph", false)) {
            poseGraph = std::make_unique<lvi_host::PoseGraphBackend>(0, p.max_keyframes, LVI_PGO_MAX_LOOPS);
            mo->usePoseGraph(poseGraph.get());
            lvi_host::GpsSettings gs;
            gs.useGpsElevation = useGpsElevation; gs.gpsCovThreshold = gpsCovThreshold; gs.poseCovThreshold = poseCovThreshold;
            mo->useGps(gs);
            subGPS = create_subscription<nav_msgs::msg::Odometry>(                                                       // :172-174
                gpsTopic, 200, [this](const nav_msgs::msg::Odometry::SharedPtr m) {
                    const double xyz[3] = {m->pose.pose.position.x, m->pose.pose.position.y, m->pose.pose.position.z};
                    const double cov[3] = {m->pose.covariance[0], m->pose.covariance[7], m->pose.covariance[14]};
                    std::lock_guard<std::mutex> lock(mtx);
                    mo->gpsHandler(stamp2Sec(m->header.stamp), xyz, cov);                                                // :334-337
                });
        }
        pubHistoryKeyFrames = create_publisher<sensor_msgs::msg::PointCloud2>("lio_sam/mapping/icp_loop_closure_history_cloud", 1);   // :239
        pubIcpKeyFrames = create_publisher<sensor_msgs::msg::PointCloud2>("lio_sam/mapping/icp_loop_closure_history_cloud", 1);       // :240 (the same topic, as written)
        pubLoopConstraintEdge = create_publisher<visualization_msgs::msg::MarkerArray>("/lio_sam/mapping/loop_closure_constraints", 1);
        subLoop = create_subscription<std_msgs::msg::Float64MultiArray>(                                                 // :175-177
            "/vins/loop/match_frame", qos, [this](const std_msgs::msg::Float64MultiArray::SharedPtr m) {
                std::lock_guard<std::mutex> lock(mtxLoopInfo);
                loop->loopInfoHandler(m->data.data(), m->data.size());
            });
        pubLaserCloudSurround = create_publisher<sensor_msgs::msg::PointCloud2>("lio_sam/mapping/map_global", 1);       // :162
        pubKeyPoses = create_publisher<sensor_msgs::msg::PointCloud2>("lio_sam/mapping/trajectory", 1);                 // :161-167
        pubLaserOdometryGlobal = create_publisher<nav_msgs::msg::Odometry>("lio_sam/mapping/odometry", qos);
        pubLaserOdometryIncremental = create_publisher<nav_msgs::msg::Odometry>("lio_sam/mapping/odometry_incremental", qos);
        pubPath = create_publisher<nav_msgs::msg::Path>("lio_sam/mapping/path", 1);
        pubRecentKeyFrames = create_publisher<sensor_msgs::msg::PointCloud2>("lio_sam/mapping/map_local", 1);           // :242
        br = std::make_unique<tf2_ros::TransformBroadcaster>(this);
        subCloud = create_subscription<lidar_odometry::msg::CloudInfo>(                                                  // :169-171
            "lio_sam/feature/cloud_info", qos, std::bind(&mapOptimization::laserCloudInfoHandler, this, std::placeholders::_1));
        srvSaveMap = create_service<lidar_odometry::srv::SaveMap>(                                                      // :179-238
            "lio_sam/save_map", [this](const std::shared_ptr<rmw_request_id_t>, const std::shared_ptr<lidar_odometry::srv::SaveMap::Request> req,
                                       std::shared_ptr<lidar_odometry::srv::SaveMap::Response> res) {
                const std::string dir = std::string(std::getenv("HOME")) + (req->destination.empty() ? savePCDDirectory : req->destination);
                RCLCPP_INFO(get_logger(), "Saving map to pcd files in %s", dir.c_str());
                res->success = saveMap(dir, req->resolution, req->resolution, req->resolution != 0, false);
            });
    }

    static pcl::PointCloud<pcl::PointXYZI>::Ptr toPcl(const std::vector<lvi_pt>& v)
    {
        pcl::PointCloud<pcl::PointXYZI>::Ptr c(new pcl::PointCloud<pcl::PointXYZI>());
        c->resize(v.size());
        for (size_t i = 0; i < v.size(); i++) { auto& q = (*c)[i]; q.x = v[i].x; q.y = v[i].y; q.z = v[i].z; q.intensity = v[i].intensity; }
        return c;
    }

    // save_map (binary: trajectory, transformations, CornerMap, SurfMap, GlobalMap; :179-236) or the shutdown save (ASCII:
    // trajectory, transformations, cloudCorner, cloudSurf, cloudGlobal; :428-457).  The fuse runs on the GPU under the node's
    // mutex; the files are written outside it.  Returns what save_map's `success` reports: the GlobalMap write.
    bool saveMap(const std::string& dir, float leafCorner, float leafSurf, bool filtered, bool ascii)
    {
        std::vector<lvi_pt> raw[2], ds[2];
        pcl::PointCloud<pcl::PointXYZI>::Ptr kp3 = nullptr;
        pcl::PointCloud<PointXYZIRPYT>::Ptr kp6(new pcl::PointCloud<PointXYZIRPYT>());
        {
            std::lock_guard<std::mutex> g(gmapMtx);
            std::lock_guard<std::mutex> lock(mtx);
            gmap->fuseAll(filtered ? leafCorner : 0.f, filtered ? leafSurf : 0.f, raw, ds);
            kp3 = toPcl(mo->cloudKeyPoses3D);
            for (const lvi_host::PointTypePose& p : mo->cloudKeyPoses6D) {
                PointXYZIRPYT q; q.x = p.x; q.y = p.y; q.z = p.z; q.intensity = p.intensity; q.roll = p.roll; q.pitch = p.pitch; q.yaw = p.yaw; q.time = p.time;
                kp6->push_back(q);
            }
        }
        std::error_code ec;
        std::filesystem::create_directories(dir, ec);
        const std::string d = dir.empty() || dir.back() == '/' ? dir : dir + "/";
        pcl::PointCloud<pcl::PointXYZI>::Ptr global = toPcl(raw[0]);
        *global += *toPcl(raw[1]);                                      // the RAW corner cloud, then the RAW surf cloud
        if (ascii) {
            pcl::io::savePCDFileASCII(d + "trajectory.pcd", *kp3);
            pcl::io::savePCDFileASCII(d + "transformations.pcd", *kp6);
            pcl::io::savePCDFileASCII(d + "cloudCorner.pcd", *toPcl(ds[0]));
            pcl::io::savePCDFileASCII(d + "cloudSurf.pcd", *toPcl(ds[1]));
            return pcl::io::savePCDFileASCII(d + "cloudGlobal.pcd", *global) == 0;
        }
        pcl::io::savePCDFileBinary(d + "trajectory.pcd", *kp3);
        pcl::io::savePCDFileBinary(d + "transformations.pcd", *kp6);
        pcl::io::savePCDFileBinary(d + "CornerMap.pcd", *toPcl(ds[0]));
        pcl::io::savePCDFileBinary(d + "SurfMap.pcd", *toPcl(ds[1]));
        return pcl::io::savePCDFileBinary(d + "GlobalMap.pcd", *global) == 0;
    }

    // publishGlobalMap (:460-510): the node's mutex is held for the key selection and the enqueue of the build only; the
    // wait for the GPU and the copy of the cloud run beside the scan path (include/lvi_gmap.h's concurrency rule)
    void publishGlobalMap()
    {
        if (pubLaserCloudSurround->get_subscription_count() == 0) return;
        std::lock_guard<std::mutex> g(gmapMtx);
        rclcpp::Time stamp;
        {
            std::lock_guard<std::mutex> lock(mtx);
            if (!gmap->startGlobalMap()) return;                                                  // no key poses
            stamp = timeLaserInfoStamp;
        }
        std::vector<lvi_pt> cloud;
        gmap->finishGlobalMap(cloud);
        publishCloud(pubLaserCloudSurround, toPcl(cloud), stamp, odometryFrame);
    }

    void visualizeGlobalMapThread()                                                                // :421-457
    {
        rclcpp::Rate rate(0.2);
        while (rclcpp::ok()) {
            rate.sleep();
            try { publishGlobalMap(); }
            catch (const std::exception& e) { RCLCPP_ERROR(get_logger(), "publishGlobalMap: %s", e.what()); }
        }
        if (!savePCD) return;
        const std::string dir = std::string(std::getenv("HOME")) + savePCDDirectory;
        std::cout << "Saving map to pcd files in " << dir << std::endl;
        saveMap(dir, mappingCornerLeafSize, mappingSurfLeafSize, true, true);
    }

    // performLoopClosure (:549-628): the node's mutex is held for the pose copies, the key search and the enqueue of the job
    // only; the wait for the GPU, the gates and the constraint run beside the scan path (include/lvi_loop.h's concurrency rule)
    void performLoopClosure()
    {
        std::lock_guard<std::mutex> g(loopMtx);
        rclcpp::Time stamp;
        {
            std::lock_guard<std::mutex> lock(mtx);
            std::lock_guard<std::mutex> li(mtxLoopInfo);
            if (!loop->startLoop()) return;                                                       // no key poses, no loop found
            stamp = timeLaserInfoStamp;
        }
        const bool pushed = loop->finishLoop();
        if (loop->lastInfo.status == LVI_LOOP_TOO_FEW_POINTS) return;                            // :572-573
        std::vector<lvi_pt> cloud;
        if (pubHistoryKeyFrames->get_subscription_count() != 0) {                                 // :574-575
            loop->fetch(LVI_LOOP_TARGET, cloud);
            publishCloud(pubHistoryKeyFrames, toPcl(cloud), stamp, odometryFrame);
        }
        if (!pushed) return;                                                                      // :592-593
        if (pubIcpKeyFrames->get_subscription_count() != 0) {                                     // :596-601
            loop->fetch(LVI_LOOP_ALIGNED, cloud);
            publishCloud(pubIcpKeyFrames, toPcl(cloud), stamp, odometryFrame);
        }
        std::lock_guard<std::mutex> q(loopQueueMtx);                                              // :620-624
        while (!loop->loopQueue.empty()) { loopConstraints.push_back(loop->loopQueue.front()); loop->loopQueue.pop_front(); }
    }

    // the constraints found since the last call, oldest first: what addLoopFactor (:1491-1508) of a GTSAM back end consumes
    std::deque<lvi_host::LoopConstraint> takeLoopConstraints()
    {
        std::lock_guard<std::mutex> q(loopQueueMtx);
        std::deque<lvi_host::LoopConstraint> out;
        out.swap(loopConstraints);
        return out;
    }

    void visualizeLoopClosure()                                                                   // :743-794
    {
        std::lock_guard<std::mutex> g(loopMtx);
        if (loop->loopIndexContainer.empty()) return;
        visualization_msgs::msg::MarkerArray markerArray;
        visualization_msgs::msg::Marker markerNode, markerEdge;
        rclcpp::Time stamp;
        { std::lock_guard<std::mutex> lock(mtx); stamp = timeLaserInfoStamp; }
        markerNode.header.frame_id = odometryFrame; markerNode.header.stamp = stamp;
        markerNode.action = visualization_msgs::msg::Marker::ADD; markerNode.type = visualization_msgs::msg::Marker::SPHERE_LIST;
        markerNode.ns = "loop_nodes"; markerNode.id = 0; markerNode.pose.orientation.w = 1;
        markerNode.scale.x = 0.3; markerNode.scale.y = 0.3; markerNode.scale.z = 0.3;
        markerNode.color.r = 0; markerNode.color.g = 0.8; markerNode.color.b = 1; markerNode.color.a = 1;
        markerEdge.header.frame_id = odometryFrame; markerEdge.header.stamp = stamp;
        markerEdge.action = visualization_msgs::msg::Marker::ADD; markerEdge.type = visualization_msgs::msg::Marker::LINE_LIST;
        markerEdge.ns = "loop_edges"; markerEdge.id = 1; markerEdge.pose.orientation.w = 1; markerEdge.scale.x = 0.1;
        markerEdge.color.r = 0.9; markerEdge.color.g = 0.9; markerEdge.color.b = 0; markerEdge.color.a = 1;
        for (const auto& kv : loop->loopIndexContainer) {
            for (int key : {kv.first, kv.second}) {
                geometry_msgs::msg::Point p;
                p.x = loop->copy_cloudKeyPoses6D[key].x; p.y = loop->copy_cloudKeyPoses6D[key].y; p.z = loop->copy_cloudKeyPoses6D[key].z;
                markerNode.points.push_back(p); markerEdge.points.push_back(p);
            }
        }
        markerArray.markers.push_back(markerNode); markerArray.markers.push_back(markerEdge);
        pubLoopConstraintEdge->publish(markerArray);
    }

    void loopClosureThread()                                                                      // :523-535
    {
        if (loopClosureEnableFlag == false) return;
        rclcpp::Rate rate(loopClosureFrequency);
        while (rclcpp::ok()) {
            rate.sleep();
            try { performLoopClosure(); visualizeLoopClosure(); }
            catch (const std::exception& e) { RCLCPP_ERROR(get_logger(), "performLoopClosure: %s", e.what()); }
        }
    }

    static void toHost(const sensor_msgs::msg::PointCloud2& msg, std::vector<lvi_pt>& out)
    {
        pcl::PointCloud<pcl::PointXYZI> c; pcl::fromROSMsg(msg, c);
        out.resize(c.size());
        for (size_t i = 0; i < c.size(); i++) out[i] = lvi_pt{c[i].x, c[i].y, c[i].z, c[i].intensity};
    }

    void laserCloudInfoHandler(const lidar_odometry::msg::CloudInfo::SharedPtr msgIn)     // :298-333
    {
        lvi_host::CloudInfo ci;
        ci.stamp = stamp2Sec(msgIn->header.stamp);
        ci.imu_available = msgIn->imu_available; ci.odom_available = msgIn->odom_available; ci.odom_reset_id = msgIn->odom_reset_id;
        ci.imu_roll_init = msgIn->imu_roll_init; ci.imu_pitch_init = msgIn->imu_pitch_init; ci.imu_yaw_init = msgIn->imu_yaw_init;
        ci.initial_guess_x = msgIn->initial_guess_x; ci.initial_guess_y = msgIn->initial_guess_y; ci.initial_guess_z = msgIn->initial_guess_z;
        ci.initial_guess_roll = msgIn->initial_guess_roll; ci.initial_guess_pitch = msgIn->initial_guess_pitch; ci.initial_guess_yaw = msgIn->initial_guess_yaw;
        toHost(msgIn->cloud_corner, ci.cloud_corner); toHost(msgIn->cloud_surface, ci.cloud_surface);
        std::lock_guard<std::mutex> lock(mtx);
        timeLaserInfoStamp = msgIn->header.stamp;
        const float* T = mo->transformTobeMapped;
        incrementalOdometryAffineFront = lvi_host::getTransformation(T[3], T[4], T[5], T[0], T[1], T[2]);          // updateInitialGuess :809
        if (poseGraph) {                                                                 // addLoopFactor's queues (:1511): what the loop thread found
            std::deque<lvi_host::LoopConstraint> found = takeLoopConstraints();
            poseGraph->takeLoops(found);
        }
        if (!mo->laserCloudInfoHandler(ci)) return;                                      // mappingProcessInterval gate; else: guess, map, match, keyframe, correctPoses
        if (mo->posesCorrected != posesCorrectedSeen) {                                   // :1641-1645: the path follows the corrected key poses
            posesCorrectedSeen = mo->posesCorrected;
            globalPath.poses.clear();                                                     // the key just saved is appended by publishFrames
            const size_t keep = mo->cloudKeyPoses6D.size() - (mo->lastSavedKeyFrame ? 1 : 0);
            for (size_t i = 0; i < keep; i++) globalPath.poses.push_back(pathPose(mo->cloudKeyPoses6D[i]));
        }
        publishOdometry(msgIn->header.stamp, ci);
        publishFrames(msgIn->header.stamp);
    }

    geometry_msgs::msg::PoseStamped pathPose(const lvi_host::PointTypePose& p) const              // updatePath :1650-1664
    {
        geometry_msgs::msg::PoseStamped ps;
        ps.header.stamp = rclcpp::Time((int64_t)(p.time * 1e9)); ps.header.frame_id = odometryFrame;
        ps.pose.position.x = p.x; ps.pose.position.y = p.y; ps.pose.position.z = p.z;
        tf2::Quaternion q; q.setRPY(p.roll, p.pitch, p.yaw);
        ps.pose.orientation.x = q.x(); ps.pose.orientation.y = q.y(); ps.pose.orientation.z = q.z(); ps.pose.orientation.w = q.w();
        return ps;
    }

    void publishOdometry(const builtin_interfaces::msg::Time& stamp, const lvi_host::CloudInfo& ci)               // :1666-1746
    {
        const float* T = mo->transformTobeMapped;
        nav_msgs::msg::Odometry laserOdometryROS;
        laserOdometryROS.header.stamp = stamp; laserOdometryROS.header.frame_id = odometryFrame; laserOdometryROS.child_frame_id = "odom_mapping";
        laserOdometryROS.pose.pose.position.x = T[3]; laserOdometryROS.pose.pose.position.y = T[4]; laserOdometryROS.pose.pose.position.z = T[5];
        tf2::Quaternion quat_tf; quat_tf.setRPY(T[0], T[1], T[2]);
        geometry_msgs::msg::Quaternion quat_msg; tf2::convert(quat_tf, quat_msg);
        laserOdometryROS.pose.pose.orientation = quat_msg;
        pubLaserOdometryGlobal->publish(laserOdometryROS);
        geometry_msgs::msg::TransformStamped tf;                                         // TF odom → lidar_link
        tf.header.stamp = stamp; tf.header.frame_id = odometryFrame; tf.child_frame_id = "lidar_link";
        tf.transform.translation.x = T[3]; tf.transform.translation.y = T[4]; tf.transform.translation.z = T[5]; tf.transform.rotation = quat_msg;
        br->sendTransform(tf);
        if (!lastIncreOdomPubFlag) {
            lastIncreOdomPubFlag = true; laserOdomIncremental = laserOdometryROS;
            increOdomAffine = lvi_host::getTransformation(T[3], T[4], T[5], T[0], T[1], T[2]);
        } else {
            const lvi_host::Affine3f back = lvi_host::getTransformation(T[3], T[4], T[5], T[0], T[1], T[2]);      // incrementalOdometryAffineBack :1342
            increOdomAffine = lvi_host::affineMul(increOdomAffine, lvi_host::affineMul(lvi_host::affineInverse(incrementalOdometryAffineFront), back));
            float x, y, z, roll, pitch, yaw;
            lvi_host::getTranslationAndEulerAngles(increOdomAffine, x, y, z, roll, pitch, yaw);
            if (ci.imu_available && std::abs(ci.imu_pitch_init) < 1.4) {                  // slerp with weight 0.1 (:1710-1726)
                tf2::Quaternion a, b; double r, p, yy;
                a.setRPY(roll, 0, 0); b.setRPY(ci.imu_roll_init, 0, 0); tf2::Matrix3x3(a.slerp(b, 0.1)).getRPY(r, p, yy); roll = r;
                a.setRPY(0, pitch, 0); b.setRPY(0, ci.imu_pitch_init, 0); tf2::Matrix3x3(a.slerp(b, 0.1)).getRPY(r, p, yy); pitch = p;
            }
            laserOdomIncremental.header.stamp = stamp; laserOdomIncremental.header.frame_id = odometryFrame; laserOdomIncremental.child_frame_id = "odom_mapping";
            laserOdomIncremental.pose.pose.position.x = x; laserOdomIncremental.pose.pose.position.y = y; laserOdomIncremental.pose.pose.position.z = z;
            tf2::Quaternion q; q.setRPY(roll, pitch, yaw);
            geometry_msgs::msg::Quaternion qm; tf2::convert(q, qm);
            laserOdomIncremental.pose.pose.orientation = qm;
            laserOdomIncremental.pose.covariance[0] = mo->last.degenerate ? 1 : 0;        // isDegenerate
        }
        pubLaserOdometryIncremental->publish(laserOdomIncremental);
    }

    void publishFrames(const builtin_interfaces::msg::Time& stamp)                        // :1748-1790 (key poses, local map, path)
    {
        if (mo->cloudKeyPoses3D.empty()) return;
        pcl::PointCloud<pcl::PointXYZI>::Ptr kp(new pcl::PointCloud<pcl::PointXYZI>());
        for (const lvi_pt& p : mo->cloudKeyPoses3D) { pcl::PointXYZI q; q.x = p.x; q.y = p.y; q.z = p.z; q.intensity = p.intensity; kp->push_back(q); }
        publishCloud(pubKeyPoses, kp, stamp, odometryFrame);
        if (pubRecentKeyFrames->get_subscription_count() != 0) {
            int32_t counts[8]; lvi_get_counts(handle->get(), counts);
            std::vector<lvi_pt> c((size_t)std::max(counts[5], 1)), s((size_t)std::max(counts[6], 1));
            lvi_cloud cc{(int32_t)c.size(), 0, c.data()}, sc{(int32_t)s.size(), 0, s.data()};
            if (lvi_get_map_ds(handle->get(), &cc, &sc) == LVI_OK) {                      // laserCloudSurfFromMapDS
                pcl::PointCloud<pcl::PointXYZI>::Ptr m(new pcl::PointCloud<pcl::PointXYZI>());
                for (int i = 0; i < sc.n; i++) { pcl::PointXYZI q; q.x = s[i].x; q.y = s[i].y; q.z = s[i].z; q.intensity = s[i].intensity; m->push_back(q); }
                publishCloud(pubRecentKeyFrames, m, stamp, odometryFrame);
            }
        }
        if (mo->lastSavedKeyFrame && pubPath->get_subscription_count() != 0) {            // updatePath :1650-1664
            globalPath.poses.push_back(pathPose(mo->cloudKeyPoses6D.back()));
            globalPath.header.stamp = stamp; globalPath.header.frame_id = odometryFrame;
            pubPath->publish(globalPath);
        }
    }
};

int main(int argc, char** argv)
{
    rclcpp::init(argc, argv);
    rclcpp::NodeOptions options; options.use_intra_process_comms(true);
    rclcpp::executors::SingleThreadedExecutor exec;
    auto MO = std::make_shared<mapOptimization>(options);
    exec.add_node(MO);
    std::thread loopthread(&mapOptimization::loopClosureThread, MO);                            // :1798
    std::thread visualizeMapThread(&mapOptimization::visualizeGlobalMapThread, MO);             // :1799
    RCLCPP_INFO(rclcpp::get_logger("rclcpp"), "\033[1;32m----> Map Optimization Started (MI355X scan matching).\033[0m");
    exec.spin();
    rclcpp::shutdown();
    loopthread.join();
    visualizeMapThread.join();                                                                  // the shutdown save runs there
    return 0;
}
