/* lvi_kf.h — pose_graph keyframes on the GPU: describe (blur, FAST, BRIEF, MEI lift) and match (Hamming).
 *
 * Restates the image work of the reference's KeyFrame constructor (pose_graph/src/keyframe.cpp:14-73:
 * computeWindowBRIEFPoint + computeBRIEFPoint) and the descriptor search of findConnection (:81-131, 266-271:
 * searchByBRIEFDes / searchInAera / HammingDis) behind an opaque handle.  Exported by liblvi_hip.so only (the CPU
 * oracle does not implement it); a separate ABI from lvi_hotpath.h, whose version it does not change.
 *
 * The arithmetic is a restatement of OpenCV 4.5.x (GaussianBlur's fixed-point path for 8-bit images, FAST-9/16 with
 * its cornerScore) and of DVision::BRIEF, all of it in integers; the parity target is tests/kfdesc_ref.py, not OpenCV
 * itself.
 *
 *   blur    GaussianBlur(u8, Size(9, 9), 2, 2): 8.8 weights {7, 17, 32, 46, 52, 46, 32, 17, 7}, BORDER_REFLECT_101,
 *           h = sum w src (u16), v = sum w h (u32), out = (v + 32768) >> 16
 *   FAST    on the unblurred image, threshold 20, 3x3 non-max suppression, keypoints in row-major order
 *   BRIEF   on the blurred image: pair i of point (px, py) reads (int)(px + (float)x1[i]) ... (f32 sum, truncated
 *           towards zero); bit i = both ends inside the image and blur[Y1][X1] < blur[Y2][X2]; a descriptor is
 *           4 x uint64, bit i in word i >> 6 at position i & 63
 *   match   per window descriptor: the lowest-index old descriptor with the smallest distance below 128; accepted
 *           when that distance is below 80
 *
 * A handle owns a device-resident keyframe store of max_keyframes slots; a slot holds the FAST keypoints (pixel and
 * normalised coordinates, descriptors) and the window points (pixel coordinates, descriptors) of one keyframe.  Old
 * keyframes stay on the GPU between describe and match.
 */
#ifndef LVI_KF_H
#define LVI_KF_H

#include "lvi_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_KF_ABI_VERSION   1
#define LVI_KF_PAIRS         256   /* BRIEF pairs = descriptor bits */
#define LVI_KF_PATTERN_MAX   24    /* |offset| bound of the pattern */
#define LVI_KF_MIN_SIDE      16    /* smallest image side */
#define LVI_KF_FAST_T        20    /* fast_th of computeBRIEFPoint */
#define LVI_KF_MATCH_START   128   /* searchInAera: bestDist starts here */
#define LVI_KF_MATCH_ACCEPT  80    /* ... and a best below this is a match */
/* soft outcome of lvi_kf_describe: FAST found more corners than max_keypoints; the first max_keypoints in row-major
 * order were stored */
#define LVI_KF_TRUNCATED     16

typedef struct lvi_kf lvi_kf;

typedef struct lvi_kf_info {
    int32_t n_keypoints_found;   /* corners after non-max suppression */
    int32_t n_keypoints_stored;  /* min(found, max_keypoints) */
    int32_t n_window;
    int32_t reserved;
} lvi_kf_info;

int32_t lvi_kf_abi_version(void);

/* x1, y1, x2, y2: the BRIEF pattern, LVI_KF_PAIRS ints each within +-LVI_KF_PATTERN_MAX */
int32_t lvi_kf_create(int32_t device, int32_t max_width, int32_t max_height, int32_t max_keypoints, int32_t max_window,
                      int32_t max_keyframes, const int32_t *x1, const int32_t *y1, const int32_t *x2, const int32_t *y2, lvi_kf **out);
void lvi_kf_destroy(lvi_kf *h);

/* The KeyFrame constructor's image work into `slot` (overwriting what it held).  img: 8-bit, `stride` bytes per row;
 * window_xy [n_window][2] = point_2d_uv (finite; may be NULL when n_window = 0); cam = the MEI model of keypoints_norm,
 * NULL stores zeros there.  Returns LVI_OK or LVI_KF_TRUNCATED; LVI_ERR_INVALID_ARG (nothing written, the slot
 * unchanged) for a bad slot, an image below 16x16 or above the handle's capacity, stride < w, or n_window > max_window.
 * One upload, one wait. */
int32_t lvi_kf_describe(lvi_kf *h, int32_t slot, const uint8_t *img, int32_t w, int32_t hgt, int32_t stride, const float *window_xy,
                        int32_t n_window, const lvi_mei_params *cam, lvi_kf_info *info_out);

/* Download a slot.  counts[2] = {n_keypoints, n_window}; the arrays hold at least that many entries (max_keypoints /
 * max_window always suffice): kp_xy, kp_norm, win_xy [n][2] float, kp_desc, win_desc [n][4] uint64.  Any pointer may be NULL. */
int32_t lvi_kf_get(lvi_kf *h, int32_t slot, int32_t counts[2], float *kp_xy, float *kp_norm, uint64_t *kp_desc, float *win_xy,
                   uint64_t *win_desc);
/* Upload a slot (a keyframe loaded from disk, the loadKeyFrame constructor); a NULL array stores zeros. */
int32_t lvi_kf_put(lvi_kf *h, int32_t slot, int32_t n_keypoints, const float *kp_xy, const float *kp_norm, const uint64_t *kp_desc,
                   int32_t n_window, const float *win_xy, const uint64_t *win_desc);
int32_t lvi_kf_release(lvi_kf *h, int32_t slot);

/* searchByBRIEFDes: the window descriptors of `cur_slot` against the keypoint descriptors of `old_slot`.  Outputs hold
 * cur's n_window entries (any may be NULL): status 1 = matched; index = the best old keypoint, -1 when no distance was
 * below 128; dist = its distance, 128 then.  Ties go to the lowest index.  LVI_ERR_INVALID_ARG for an empty or released
 * slot (nothing written).  One launch, one download, one wait. */
int32_t lvi_kf_match(lvi_kf *h, int32_t cur_slot, int32_t old_slot, uint8_t *status_out, int32_t *index_out, int32_t *dist_out);

/* ---- debug view (tests) ------------------------------------------------------------------------- */
/* the blurred image and the FAST score map of the last describe, [hgt][w] tightly packed; wh_out[2] = {w, hgt} */
int32_t lvi_kf_debug_maps(lvi_kf *h, uint8_t *blur, uint8_t *score, int32_t wh_out[2]);

#ifdef __cplusplus
}
#endif
#endif /* LVI_KF_H */
