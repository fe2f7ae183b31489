/* lvi_gmap.h — mapOptimization's global map on the GPU: the fused keyframe clouds and one VoxelGrid.
 *
 * Restates the fuse + filter of publishGlobalMap (mapOptimization.cpp:460-510: corner_k then surf_k per key through
 * transformPointCloud with cloudKeyPoses6D[k], then VoxelGrid globalMapVisualizationLeafSize) and of the save_map
 * service / the shutdown save (:179-236, :428-457: corner and surf fused separately, each with its own VoxelGrid).
 * The clouds come from the device keyframe store of an lvi_lidar handle (lvi_keyframe_add*): nothing travels
 * through the host but the key list and the result the caller asks for.
 *
 * Exported by liblvi_hip.so only (the CPU oracle does not implement it); a separate ABI from lvi_hotpath.h, whose
 * version it does not change.
 *
 * Arena.  lvi_gmap_reserve creates, on first use, the fused cloud and a VoxelGrid plan for max_points points, apart
 * from the local map's buffers: a handle that never calls it allocates nothing more.  lvi_gmap_arena_bytes reports its
 * size (about 100 B per reserved point).
 *
 * Streams.  lvi_gmap_build enqueues on a stream of its own and returns without waiting for the work: the reference runs
 * it on a thread of its own, and the scan path must not wait for a multi-ms build.  That stream first waits for
 * everything enqueued on the handle's main stream so far (the keyframe copies of lvi_keyframe_add_current).  Poses are
 * read from the store when the build is enqueued: a later lvi_keyframe_set_pose changes later builds only.
 *
 * Concurrency.  lvi_gmap_result and lvi_gmap_fetch may run on another host thread concurrently with any other call on
 * the handle, except lvi_gmap_build, lvi_gmap_reserve, lvi_gmap_release, lvi_keyframes_clear and lvi_lidar_destroy.
 * Those five are called from the thread that owns the handle (or under its lock); the last four wait for a build in
 * flight.  result and fetch are called from one thread at a time.  Errors are reported per thread (lvi_last_error),
 * and the build's launches are not profiled (lvi_prof_*), so no state is shared with the scan path.
 */
#ifndef LVI_GMAP_H
#define LVI_GMAP_H

#include "lvi_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_GMAP_ABI_VERSION 1
#define LVI_GMAP_MAX_POINTS  (1 << 25)   /* largest reservation: the VoxelGrid plan's limit (csrc/lvi_voxel.hpp) */

enum {
    LVI_GMAP_CORNER = 0,                 /* corner clouds of the listed keys, in list order (save_map's CornerMap) */
    LVI_GMAP_SURF = 1,                   /* surf clouds, in list order (SurfMap) */
    LVI_GMAP_CORNER_SURF = 2             /* per key corner_k then surf_k (publishGlobalMap's globalMapKeyFrames) */
};
enum { LVI_GMAP_FUSED = 0, LVI_GMAP_FILTERED = 1 };

typedef struct lvi_gmap_info {
    int32_t n_fused;                     /* points of the fused cloud */
    int32_t n_out;                       /* points of the filtered cloud (= n_fused when overflow or leaf == 0) */
    int32_t overflow;                    /* PCL's "leaf size too small" rule fired: the filtered cloud IS the fused cloud */
    int32_t filtered;                    /* leaf > 0 */
} lvi_gmap_info;

int32_t lvi_gmap_abi_version(void);

/* the arena for fused clouds of up to max_points points (1..LVI_GMAP_MAX_POINTS); a smaller or equal reservation than
 * the current one is a no-op, a larger one replaces it (waits for a build in flight) */
int32_t lvi_gmap_reserve(lvi_lidar *h, int32_t max_points);
/* frees the arena (waits for a build in flight); a later build needs a new reservation */
int32_t lvi_gmap_release(lvi_lidar *h);
int32_t lvi_gmap_arena_bytes(lvi_lidar *h, int64_t *bytes);

/* fuse the listed keyframes (duplicates allowed) of the store and filter the result.  which: LVI_GMAP_*.  leaf == 0: no
 * filter; leaf < 0 or NaN, a key out of range, a bad `which`: LVI_ERR_INVALID_ARG.  No reservation: LVI_ERR_STATE.  A
 * fused cloud above the reservation or a key list above the segment table (2 * max_keyframes + 2048 clouds):
 * LVI_ERR_CAPACITY.  Every error leaves all state as it was (the previous build's result stays readable).  *n_fused
 * (optional) = the fused size, known on the host.  Waits only for a previous build still in flight. */
int32_t lvi_gmap_build(lvi_lidar *h, const int32_t *keys, int32_t n_keys, int32_t which, float leaf, int32_t *n_fused);
/* waits for the last build (its stream only) and reports its sizes; LVI_ERR_STATE before the first build */
int32_t lvi_gmap_result(lvi_lidar *h, lvi_gmap_info *info);
/* copies points [first, first + count) of the fused or filtered cloud of the last build into pageable host memory,
 * through a small pinned double buffer (implies lvi_gmap_result).  The range must lie in the cloud. */
int32_t lvi_gmap_fetch(lvi_lidar *h, int32_t what, int32_t first, int32_t count, lvi_pt *out);
/* the last build's voxel keys (tests): every fused point's PCL linear voxel idx under the last filter's grid, recomputed
 * on the device and grouped on the host — the distinct idx ascending (PCL's output order) and the points of each.  It
 * checks the grid (bbox, key expression), not the filter's compaction, whose output lvi_gmap_fetch returns.  *n_out =
 * voxels (0 when no filter ran or the overflow rule fired) whatever cap is.  Same thread rule as lvi_gmap_build. */
int32_t lvi_gmap_debug_voxel(lvi_lidar *h, int32_t *cells, int32_t *counts, int32_t cap, int32_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* LVI_GMAP_H */
