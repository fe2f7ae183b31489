/* lvi_pnp.h — the pose graph's loop confirmation (KeyFrame::PnPRANSAC) on the GPU.
 *
 * Restates OpenCV 4.5.x cv::solvePnPRansac(matched_3d, matched_2d_old_norm, K = I, D = empty, rvec, t, true, 100,
 * 10.0 / 460.0, 0.99, inliers) — the call of keyframe.cpp:163 — behind an opaque handle, reduced to what
 * KeyFrame::findConnection (keyframe.cpp:179-211) reads afterwards: the inlier status of keyframe.cpp:167-174.  rvec and t
 * are never read there, so the extrinsic guess is not an input and the final iterative refit is not restated.
 * EPnP on 5 points per hypothesis (calib3d/src/epnp.cpp), RANSAC for n >= 6 (ptsetreg.cpp), EPnP on all points for
 * n == 5.  DESIGN §16 is the contract; parity is against that restatement (tests/pnp_ref.py), not against OpenCV itself.
 * Exported by liblvi_hip.so only (the CPU oracle does not implement it); a separate ABI from lvi_hotpath.h, whose version
 * it does not change.
 *
 * One call = one correspondence set in host memory: one upload, two kernels, one download of the status bytes (and the
 * info record).  The random-sample stream (cv::RNG + getSubset) is sequential integer work and is generated on the host
 * inside the call.
 */
#ifndef LVI_PNP_H
#define LVI_PNP_H

#include "lvi_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_PNP_ABI_VERSION    1
#define LVI_PNP_MAX_POINTS     2048   /* upper bound of max_points */
#define LVI_PNP_MAX_ITERS      1024   /* upper bound of max_iters */

/* lvi_pnp_info.path (whether a model was found: best_iter >= 0) */
#define LVI_PNP_PATH_DIRECT    1      /* n == 5: EPnP on all five points; status all ones when a model results */
#define LVI_PNP_PATH_RANSAC    2      /* n >= 6 */

typedef struct lvi_pnp lvi_pnp;

typedef struct lvi_pnp_info {
    int32_t path;          /* LVI_PNP_PATH_* */
    int32_t iters;         /* iterations the walk ran (RANSACPointSetRegistrator::run, ptsetreg.cpp) */
    int32_t n_subsets;     /* subsets the sample stream produced: max_iters, or 1 on the direct path */
    int32_t best_iter;     /* iteration of the chosen hypothesis; -1 = no model, the status is all zeros */
    int32_t n_inliers;     /* ones in the status */
    int32_t which_beta;    /* 1..3: the beta initialisation epnp::compute_pose chose; 0 when no model */
    double  R[9];          /* the chosen hypothesis, row-major; zeros when none */
    double  t[3];
    double  stream_us;     /* host time of the sample stream (cv::RNG + getSubset) of this call */
} lvi_pnp_info;

int32_t lvi_pnp_abi_version(void);

/* max_points: largest n of one call (5..LVI_PNP_MAX_POINTS); max_iters: solvePnPRansac's iterationsCount
 * (1..LVI_PNP_MAX_ITERS; keyframe.cpp:163 passes 100). */
int32_t lvi_pnp_create(int32_t device, int32_t max_points, int32_t max_iters, lvi_pnp **out);
void lvi_pnp_destroy(lvi_pnp *h);

/* pts3d_xyz [n][3] float (matched_3d), pts2d_xy [n][2] float (matched_2d_old_norm).  threshold: reprojectionError, read
 * as the `float` parameter it is (keyframe.cpp:163 passes 10.0 / 460.0); confidence: 0.99 there.  status_out [n]:
 * 1 = inlier (keyframe.cpp:167-174).  info_out may be NULL.  n < 5 (OpenCV switches to P3P at n == 4, which is not
 * restated; findConnection only calls with n > 25, keyframe.cpp:200), n > max_points or a NULL pointer:
 * LVI_ERR_INVALID_ARG and nothing is written.  One wait. */
int32_t lvi_pnp_solve(lvi_pnp *h, const float *pts3d_xyz, const float *pts2d_xy, int32_t n, double threshold, double confidence,
                      uint8_t *status_out, lvi_pnp_info *info_out);

/* ---- introspection of the last lvi_pnp_solve (tests) ----------------------------------------------
 * subsets [cap][5]: the sample stream; has_model [cap]: 0 = the hypothesis's control points were singular;
 * Rt [cap][12]: R row-major, then t; good [cap]: the hypothesis's inlier count.  Any pointer may be NULL; *n_out = the number of hypotheses (n_subsets). */
int32_t lvi_pnp_trace(lvi_pnp *h, int32_t *subsets, int32_t *has_model, double *Rt, int32_t *good, int32_t cap, int32_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* LVI_PNP_H */
