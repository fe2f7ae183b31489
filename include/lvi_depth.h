/* lvi_depth.h — LiDAR depth association of the feature tracker on the GPU.
 *
 * Restates the reference's feature_tracker_node.cpp lidar_callback (:273-377: a window of
 * LiDAR clouds, VoxelGrid 0.2, field-of-view cut, world frame, fused and VoxelGrid 0.2
 * again) and DepthRegister::get_depth (feature_tracker.h:116-331: 360x360 range image,
 * unit sphere, 3 nearest neighbours, ray/plane intersection) behind an opaque handle.
 * Exported by liblvi_hip.so only (the CPU oracle does not implement it); a separate ABI
 * from lvi_hotpath.h, whose version it does not change.
 *
 * Poses: pose6 = {x, y, z, roll, pitch, yaw} of the body in the world frame (what the node
 * reads from TF vins_world <- vins_body_ros), turned into pcl::getTransformation in f32.
 * NULL = no transform available: the callback returns after counting the cloud, get_depth
 * returns -1 for every feature.  Neither touches the GPU then.
 */
#ifndef LVI_DEPTH_H
#define LVI_DEPTH_H

#include "lvi_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_DEPTH_ABI_VERSION 1
#define LVI_DEPTH_BINS        360   /* num_bins: rows and columns of the range image */
#define LVI_DEPTH_MAX_CLOUDS  128   /* upper bound of max_clouds (window length in clouds) */

typedef struct lvi_depth lvi_depth;

int32_t lvi_depth_abi_version(void);

/* max_clouds: clouds the window may hold at once (1..LVI_DEPTH_MAX_CLOUDS); max_cloud_points:
 * points of one incoming cloud; max_features: features of one get_depth call; lidar_skip:
 * LIDAR_SKIP of the camera config; window_s: the queue's age limit (5.0 in the reference). */
int32_t lvi_depth_create(int32_t device, int32_t max_clouds, int32_t max_cloud_points, int32_t max_features, int32_t lidar_skip,
                         double window_s, lvi_depth **out);
void lvi_depth_destroy(lvi_depth *h);

/* lidar_callback: one incoming cloud (sensor frame, host memory) with its stamp.  *used (optional)
 * = 1 when the cloud entered the window, 0 when it was skipped or had no pose.  LVI_ERR_CAPACITY
 * when n > max_cloud_points (nothing changes) or when the window would hold more than max_clouds
 * clouds (nothing changes but the skip counter, which the reference advances first).  One wait. */
int32_t lvi_depth_lidar_cloud(lvi_depth *h, const lvi_pt *pts, int32_t n, const float pose6[6], double stamp, int32_t *used);
/* the same for a cloud already in device memory of the handle's GPU (e.g. a deskewed scan) */
int32_t lvi_depth_lidar_cloud_device(lvi_depth *h, const lvi_pt *d_pts, int32_t n, const float pose6[6], double stamp, int32_t *used);

/* get_depth: features_xyz [n][3] = the published points (un_x, un_y, 1); depth_out [n] = the
 * message's depth channel (> 3.0, else -1).  n = 0 is valid.  One wait per call. */
int32_t lvi_depth_get(lvi_depth *h, const float pose6[6], const float *features_xyz, int32_t n, float *depth_out);

/* ---- state and debug views (tests) ------------------------------------------------------------- */
/* state[4]: clouds in the window, skip counter (lidar_count), depth cloud points, clouds used so far */
int32_t lvi_depth_state(lvi_depth *h, int32_t state[4]);
/* replace the depth cloud (world frame) as if the window had produced it; n <= max_clouds * max_cloud_points */
int32_t lvi_depth_set_cloud(lvi_depth *h, const lvi_pt *pts, int32_t n);
/* the current depth cloud; *n_out = its size whatever cap is */
int32_t lvi_depth_get_cloud(lvi_depth *h, lvi_pt *out, int32_t cap, int32_t *n_out);
/* the last window fusion's VoxelGrid: distinct voxel idx in output order and points per voxel */
int32_t lvi_depth_debug_voxel(lvi_depth *h, int32_t *cells, int32_t *counts, int32_t cap, int32_t *n_out);
/* the last get_depth's range image: depth-cloud index kept per bin, row-major [360][360], -1 = empty */
int32_t lvi_depth_debug_range(lvi_depth *h, int32_t *sel);
/* the last get_depth's unit-sphere cloud in row-major bin order (intensity = range) */
int32_t lvi_depth_debug_sphere(lvi_depth *h, lvi_pt *out, int32_t cap, int32_t *n_out);
/* the last get_depth's neighbours: idx [n][3] into the sphere cloud (-1 = none) and their squared
 * distances, sorted; all -1 when the call did not search (no pose, fewer than 10 sphere points) */
int32_t lvi_depth_debug_neighbors(lvi_depth *h, int32_t *idx, float *sqd, int32_t cap, int32_t *n_out);
/* 1: search every row instead of the band around the feature's row (the band's test) */
int32_t lvi_depth_set_full_search(lvi_depth *h, int32_t on);

#ifdef __cplusplus
}
#endif
#endif /* LVI_DEPTH_H */
