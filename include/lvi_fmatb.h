/* lvi_fmatb.h — rejectWithF's outlier rejection for all cameras of a rig in one call.
 *
 * Up to LVI_TRACKER_MAX_BATCH independent point-pair sets ("slots") go through the
 * cv::findFundamentalMat(pts1, pts2, FM_RANSAC, threshold, confidence, maxIters, status) of
 * feature_tracker.cpp:229 as include/lvi_fmat.h restates it, on one stream and with
 * one wait.  Every slot's status, info record and trace are bit-identical to those of a separate
 * lvi_fmat handle given the same inputs.  DESIGN §25 is the contract.  Exported by liblvi_hip.so
 * only; a separate ABI from lvi_fmat.h, lvi_tbatch.h and lvi_hotpath.h, whose versions it does not
 * change.
 *
 * One call: per active slot, in slot order, the host draws the slot's sample stream and enqueues
 * the slot's upload and one launch that scores its hypotheses, without waiting, so the device
 * scores slot s while the host draws slot s + 1.  Then one launch walks all slots, one download
 * returns every slot's status and info, and the host waits once.
 */
#ifndef LVI_FMATB_H
#define LVI_FMATB_H

#include "lvi_fmat.h"     /* lvi_fmat_info, LVI_FMAT_MAX_POINTS, LVI_FMAT_MAX_ITERS, LVI_FMAT_PATH_* */
#include "lvi_tbatch.h"   /* LVI_TRACKER_MAX_BATCH */

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_FMATB_ABI_VERSION   1

typedef struct lvi_fmatb lvi_fmatb;

int32_t lvi_fmatb_abi_version(void);

/* feature_tracker.cpp:229, once per slot: lvi_fmat_create `slots` times (1..LVI_TRACKER_MAX_BATCH)
 * with the same max_points (7..LVI_FMAT_MAX_POINTS) and max_iters (1..LVI_FMAT_MAX_ITERS), on one
 * stream and one pair of pinned blocks. */
int32_t lvi_fmatb_create(int32_t device, int32_t slots, int32_t max_points, int32_t max_iters, lvi_fmatb **out);
/* feature_tracker.cpp:229: lvi_fmat_destroy for all slots. */
void lvi_fmatb_destroy(lvi_fmatb *h);

/* feature_tracker.cpp:229's checkSubset: lvi_fmat_set_check_subset for all slots. */
int32_t lvi_fmatb_set_check_subset(lvi_fmatb *h, int32_t mode);

/* feature_tracker.cpp:229 for every slot: lvi_fmat_find per slot.  All tables have `slots` entries.
 * n[s] == -1: slot s sits out — its pointers are not read, status_out[s] is not written,
 * info_out[s] is zeroed and its trace is empty.  Otherwise n[s] is 7..max_points, pts1_xy[s] and
 * pts2_xy[s] are [n[s]][2] float, status_out[s] is [n[s]], and threshold[s] and confidence take
 * lvi_fmat_find's defaults.  info_out ([slots]) may be NULL.
 * Every argument of every slot is checked before anything is written, staged or launched: a bad
 * value in any slot is LVI_ERR_INVALID_ARG, and no output and no slot's trace changes.
 * All slots sitting out: LVI_OK without a launch or a wait.
 * Launches: one per active slot whose sample stream is not empty, plus one; one wait. */
int32_t lvi_fmatb_find(lvi_fmatb *h, const float *const *pts1_xy, const float *const *pts2_xy, const int32_t *n, const double *threshold,
                       double confidence, uint8_t *const *status_out, lvi_fmat_info *info_out);

/* feature_tracker.cpp:229, introspection: lvi_fmat_trace for slot `slot` of the last lvi_fmatb_find
 * that returned LVI_OK.  A slot that sat out: *n_out = 0. */
int32_t lvi_fmatb_trace(lvi_fmatb *h, int32_t slot, int32_t *subsets, int32_t *nmodels, double *F, int32_t *score, int32_t cap, int32_t *n_out);

/* feature_tracker.cpp:229, bookkeeping: totals since lvi_fmatb_create (any pointer may be NULL).
 * calls: lvi_fmatb_find calls that returned LVI_OK with at least one active slot;
 * hyp_launches: one per active slot with a non-empty sample stream (a slot whose stream is empty —
 * getSubset failed at once, e.g. a collinear set — counts as active but adds no launch);
 * walk_launches and waits: one each per counted call. */
int32_t lvi_fmatb_counters(lvi_fmatb *h, int64_t *calls, int64_t *hyp_launches, int64_t *walk_launches, int64_t *waits);

#ifdef __cplusplus
}
#endif
#endif /* LVI_FMATB_H */
