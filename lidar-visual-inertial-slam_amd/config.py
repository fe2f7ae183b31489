"""YAML loader of the harness: the reference's two configuration files → the C-ABI parameter structs.

    params_lidar.yaml   (ROS 2 parameter file: /**: ros__parameters: …)   → lvi_lidar_params fields + the caller-loop settings
    params_camera.yaml  (OpenCV FileStorage yaml: %YAML:1.0, !!opencv-matrix) → lvi_tracker_params fields, MEI camera, FREQ, …

Only keys the hot path reads are mapped (utility.h:156-313, feature_tracker/src/parameters.cpp:53-110)."""
import re

import yaml

LIDAR_KEYS = ("N_SCAN", "Horizon_SCAN", "downsampleRate", "lidarMinRange", "lidarMaxRange", "edgeThreshold", "surfThreshold",
              "edgeFeatureMinValidNum", "surfFeatureMinValidNum", "odometrySurfLeafSize", "mappingCornerLeafSize", "mappingSurfLeafSize",
              "z_tollerance", "rotation_tollerance", "imuRPYWeight", "numberOfCores")
CALLER_KEYS = dict(useImuHeadingInitialization="use_imu_heading_initialization", mappingProcessInterval="mapping_process_interval",
                   surroundingkeyframeAddingDistThreshold="keyframe_adding_dist", surroundingkeyframeAddingAngleThreshold="keyframe_adding_angle",
                   surroundingKeyframeDensity="keyframe_density", surroundingKeyframeSearchRadius="keyframe_search_radius")


def load_lidar_yaml(path):
    """→ (lidar params overrides for lidar.default_params, lvh_seq_params overrides for host_api.SequentialMapper, everything else)"""
    doc = yaml.safe_load(open(path))
    node = doc
    for k in ("/**", "ros__parameters"):
        node = node[k]
    lidar = {k: node[k] for k in LIDAR_KEYS if k in node}
    caller = {v: (int(node[k]) if isinstance(node[k], bool) else node[k]) for k, v in CALLER_KEYS.items() if k in node}
    rest = {k: v for k, v in node.items() if k not in lidar and k not in CALLER_KEYS}
    return lidar, caller, rest


LOOP_KEYS = dict(loopClosureEnableFlag="enable", loopClosureFrequency="frequency", historyKeyframeSearchRadius="search_radius",
                 historyKeyframeSearchTimeDiff="search_time_diff", historyKeyframeSearchNum="search_num", historyKeyframeFitnessScore="fitness_score")


def load_loop_yaml(path):
    """→ the loop-closure settings of params_lidar.yaml (utility.h:281-286): dict(enable, frequency, search_radius,
    search_time_diff, search_num, fitness_score, surf_leaf), the settings of host_api.LoopCloser and of the loop thread;
    surf_leaf = mappingSurfLeafSize, the submaps' VoxelGrid"""
    node = yaml.safe_load(open(path))
    for k in ("/**", "ros__parameters"):
        node = node[k]
    out = {v: node[k] for k, v in LOOP_KEYS.items()}
    out["enable"] = bool(out["enable"])
    out["search_num"] = int(out["search_num"])
    for k in ("frequency", "search_radius", "search_time_diff", "fitness_score"):
        out[k] = float(out[k])
    out["surf_leaf"] = float(node["mappingSurfLeafSize"])
    return out


GPS_KEYS = dict(useGpsElevation=("use_gps_elevation", False), gpsCovThreshold=("gps_cov_threshold", 2.0), poseCovThreshold=("pose_cov_threshold", 25.0))


def load_gps_yaml(path):
    """→ the GPS settings of params_lidar.yaml (utility.h:178-183): dict(use_gps_elevation, gps_cov_threshold,
    pose_cov_threshold, gps_topic), the keyword arguments of host_api.SequentialMapper.useGps plus the topic.  The shipped
    file sets none of the three, so an absent key takes the default utility.h declares"""
    node = yaml.safe_load(open(path))
    for k in ("/**", "ros__parameters"):
        node = node[k]
    out = {name: node.get(k, default) for k, (name, default) in GPS_KEYS.items()}
    out["use_gps_elevation"] = bool(out["use_gps_elevation"])
    for k in ("gps_cov_threshold", "pose_cov_threshold"):
        out[k] = float(out[k])
    out["gps_topic"] = str(node.get("gpsTopic", "lio_sam/odometry/gps"))                # utility.h:164
    return out


def _opencv_yaml(path):
    txt = open(path).read()
    txt = re.sub(r"^%YAML[:\s]*1\.0\s*$", "", txt, flags=re.M)          # FileStorage header is not YAML 1.1 directive syntax
    txt = txt.replace("!!opencv-matrix", "")                            # plain mappings (rows / cols / dt / data)
    return yaml.safe_load(txt)


def load_camera_yaml(path):
    """→ (tracker params overrides, MEI camera dict or None, node settings: freq, F_threshold, equalize, fisheye, image size)"""
    d = _opencv_yaml(path)
    tracker = dict(max_width=int(d["image_width"]), max_height=int(d["image_height"]), max_cnt=int(d["max_cnt"]), min_dist=float(d["min_dist"]))
    cam = None
    if str(d.get("model_type", "")).upper() == "MEI":
        cam = dict(xi=float(d["mirror_parameters"]["xi"]), **{k: float(d["distortion_parameters"][k]) for k in ("k1", "k2", "p1", "p2")},
                   **{k: float(d["projection_parameters"][k]) for k in ("gamma1", "gamma2", "u0", "v0")})
    node = dict(freq=int(d["freq"]) or 100, F_threshold=float(d["F_threshold"]), equalize=int(d["equalize"]), fisheye=int(d["fisheye"]),
                image_width=int(d["image_width"]), image_height=int(d["image_height"]), image_topic=d["image_topic"], point_cloud_topic=d["point_cloud_topic"])
    return tracker, cam, node


def load_camera_lidar_yaml(path):
    """→ the lidar depth settings of the camera yaml (parameters.cpp: USE_LIDAR, LIDAR_SKIP, POINT_CLOUD_TOPIC):
    dict(use_lidar, lidar_skip, point_cloud_topic), the keyword arguments of the depth register and the node"""
    d = _opencv_yaml(path)
    return dict(use_lidar=int(d["use_lidar"]), lidar_skip=int(d["lidar_skip"]), point_cloud_topic=str(d["point_cloud_topic"]))


def load_estimator_yaml(path):
    """→ what the marginalisation reads of the camera yaml (vins_estimator's parameters.cpp:79, 120-135): dict(estimate_td,
    td, rolling_shutter_tr (0 without a rolling shutter), image_height, and the lvi_marg_params tr_over_row = TR / ROW and
    half_row = ROW / 2)"""
    d = _opencv_yaml(path)
    row = float(d["image_height"])
    tr = float(d["rolling_shutter_tr"]) if int(d.get("rolling_shutter", 0)) else 0.0
    return dict(estimate_td=bool(int(d["estimate_td"])), td=float(d["td"]), rolling_shutter_tr=tr, image_height=row, tr_over_row=tr / row, half_row=row / 2)


def load_window_yaml(path):
    """→ what the window solve reads of the camera yaml (vins_estimator's parameters.cpp): dict(max_solver_time (seconds),
    max_num_iterations, estimate_extrinsic (0 fixed, 1 refined, 2 calibrated from scratch), estimate_td, acc_n, gyr_n, acc_w,
    gyr_w, g_norm, and G = [0, 0, g_norm], the lvi_win_params gravity before the initialisation aligns it)"""
    d = _opencv_yaml(path)
    g = float(d["g_norm"])
    return dict(max_solver_time=float(d["max_solver_time"]), max_num_iterations=int(d["max_num_iterations"]), estimate_extrinsic=int(d["estimate_extrinsic"]),
                estimate_td=bool(int(d["estimate_td"])), acc_n=float(d["acc_n"]), gyr_n=float(d["gyr_n"]), acc_w=float(d["acc_w"]), gyr_w=float(d["gyr_w"]),
                g_norm=g, G=[0.0, 0.0, g])


def load_brief_pattern(path):
    """→ (x1, y1, x2, y2): the BRIEF pair offsets of support_files/brief_pattern.yml (OpenCV FileStorage yaml; what
    BriefExtractor's constructor reads, keyframe.cpp:273-291), 256 ints each within ±24: the pattern argument of
    kf.KeyframeDescriber"""
    d = _opencv_yaml(path)
    out = []
    for k in ("x1", "y1", "x2", "y2"):
        v = d.get(k)
        if not isinstance(v, list) or len(v) != 256:
            raise ValueError(f"{path}: {k} must hold 256 entries")
        if any(isinstance(e, bool) or not isinstance(e, int) or abs(e) > 24 for e in v):
            raise ValueError(f"{path}: {k} must hold integers within ±24")
        out.append([int(e) for e in v])
    return tuple(out)
