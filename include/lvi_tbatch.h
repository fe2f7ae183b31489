/* lvi_tbatch.h — up to 8 independent feature-tracker states ("slots") behind one handle, one arena and one stream.
 *
 * The batch form of the staged lvi_tracker_* interface of lvi_hotpath.h: every stage (CLAHE, pyramid level, LK, mask
 * raster, min-eigenvalue map, candidate count / emit, the LDS sort + pick, the frame-end concatenation and the MEI
 * lift) is ONE launch for all slots, the slot carried in blockIdx.z, as lvi_lidar_params.batch_scans does for scans.
 * Every slot's results are bit-identical to those of an lvi_tracker created with the same parameters and given the
 * same calls.  The reference compiles NUM_OF_CAM = 1 (feature_tracker_node.cpp:136-166 loops over trackerData[i] for
 * i < NUM_OF_CAM): this is a capability of the library for camera rigs, several robots on one device or sharded
 * replay — it does not reproduce a reference behaviour.
 *
 * Exported by liblvi_hip.so only (the CPU oracle does not implement it); a separate ABI from lvi_hotpath.h, whose
 * version it does not change.
 *
 * Per-slot arguments are tables of length `slots`.  A NULL image / n < 0 / max_corners < 0 means "this slot sits this
 * call out": its state is untouched (a slot that sits a push out keeps its cur/forw pair).  Arguments are validated
 * before the device is touched, and a call that fails a check for one slot changes no slot.
 *
 * Left out: the full-mask upload (lvi_tracker_set_mask), the one-call forms (lvi_lk_track, lvi_good_features,
 * lvi_clahe), the blocking lvi_tracker_run_gftt / lvi_tracker_get_gftt pair and a batched lvi_undistort_points.
 */
#ifndef LVI_TBATCH_H
#define LVI_TBATCH_H

#include "lvi_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_TBATCH_ABI_VERSION 1
#define LVI_TRACKER_MAX_BATCH  8

/* lvi_tbatch_debug_get: the LVI_TDBG_* items of lvi_tracker_debug_get for one slot, plus: */
#define LVI_TBDBG_REDO_MASK    100   /* i32[1] bit s = slot s's GFTT was redone in the radix form during the last frame end; `slot` is ignored */

typedef struct lvi_tbatch lvi_tbatch;

int32_t lvi_tbatch_abi_version(void);

/* lvi_tracker_create, `slots` times (1..LVI_TRACKER_MAX_BATCH) with the same parameters.  LVI_GFTT_RADIX=1 is read here, as there. */
int32_t lvi_tbatch_create(const lvi_tracker_params *p, int32_t slots, int32_t device, lvi_tbatch **out);
/* lvi_tracker_destroy */
void lvi_tbatch_destroy(lvi_tbatch *b);
/* lvi_tracker_sync */
int32_t lvi_tbatch_sync(lvi_tbatch *b);
/* lvi_tracker_set_equalize, for all slots */
int32_t lvi_tbatch_set_equalize(lvi_tbatch *b, int32_t on, double clip_limit, int32_t tiles_x, int32_t tiles_y);

/* lvi_tracker_push_image: imgs[slots]; all images of one call share w, h, stride; imgs[s] == NULL sits out. */
int32_t lvi_tbatch_push_images(lvi_tbatch *b, const uint8_t *const *imgs, int32_t w, int32_t h, int32_t stride);
/* lvi_tracker_set_points: cur_xy[slots], n[slots]; n[s] < 0 sits out. */
int32_t lvi_tbatch_set_points(lvi_tbatch *b, const float *const *cur_xy, const int32_t *n);
/* lvi_tracker_run_lk for the slots whose last set_points came after their last run_lk; LVI_ERR_STATE (and nothing runs)
 * when one of them has no image pair. */
int32_t lvi_tbatch_run_lk(lvi_tbatch *b);
/* lvi_tracker_get_lk of one slot.  The first call after lvi_tbatch_run_lk waits for the stream; the calls for the other
 * slots only copy from pinned memory. */
int32_t lvi_tbatch_get_lk(lvi_tbatch *b, int32_t slot, float *forw_xy, uint8_t *status, float *err, int32_t capacity, int32_t *n);
/* lvi_tracker_set_mask_circles: centers_xy[slots], n[slots] (n[s] < 0 sits out), one radius. */
int32_t lvi_tbatch_set_mask_circles(lvi_tbatch *b, const float *const *centers_xy, const int32_t *n, int32_t radius);
/* lvi_tracker_run_gftt_async: max_corners[slots]; max_corners[s] < 0 sits out. */
int32_t lvi_tbatch_run_gftt_async(lvi_tbatch *b, const int32_t *max_corners);
/* lvi_tracker_finish_frame: the ONE wait of the frame end for all slots.  cams[slots] or NULL; kept_xy[slots], n_kept[slots]
 * (n_kept[s] < 0 sits out); new_xy[slots] (each new_capacity pairs; entries may be NULL), n_new[slots], un_xy[slots] (or NULL;
 * entries may be NULL).  A slot whose LDS sort + pick reported an overflow is redone alone in the radix form and re-read; the
 * other slots' results stand.  A capacity error found in a slot's RESULT (more corners than max_features / new_capacity) is
 * returned after every slot has been served; the other slots' outputs are valid. */
int32_t lvi_tbatch_finish_frame(lvi_tbatch *b, const lvi_mei_params *cams, const float *const *kept_xy, const int32_t *n_kept,
                                float *const *new_xy, int32_t new_capacity, int32_t *n_new, float *const *un_xy);
/* lvi_tracker_debug_get of one slot (LVI_TDBG_*), or LVI_TBDBG_REDO_MASK */
int32_t lvi_tbatch_debug_get(lvi_tbatch *b, int32_t slot, int32_t what, void *dst, int64_t capacity_bytes, int64_t *n_bytes);
/* lvi_tracker_prof_enable / lvi_tracker_prof_reset / lvi_tracker_prof_read: one profiler for the handle (a launch serves all slots) */
int32_t lvi_tbatch_prof_enable(lvi_tbatch *b, int32_t on);
int32_t lvi_tbatch_prof_reset(lvi_tbatch *b);
int32_t lvi_tbatch_prof_read(lvi_tbatch *b, lvi_kernel_stat *stats, int32_t capacity, int32_t *n);

#ifdef __cplusplus
}
#endif
#endif /* LVI_TBATCH_H */
