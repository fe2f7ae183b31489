/* lvi_fmat.h — the feature tracker's outlier rejection (rejectWithF) on the GPU.
 *
 * Restates OpenCV 4.5.x cv::findFundamentalMat(pts1, pts2, FM_RANSAC, threshold, confidence,
 * maxIters = 1000, status) — the call of feature_tracker.cpp:229 — behind an opaque handle:
 * 7-point kernel, RANSAC for n >= 15, LMeDS for 8 <= n < 15, the kernel alone for n == 7.
 * DESIGN §11 is the contract; parity is against that restatement, not against OpenCV itself.
 * Exported by liblvi_hip.so only (the CPU oracle does not implement it); a separate ABI from
 * lvi_hotpath.h, whose version it does not change.
 *
 * One call = one point-pair set in host memory: one upload, two kernels, one download of the
 * status bytes (and the info record).  The random-sample stream (cv::RNG + getSubset) is
 * sequential integer work and is generated on the host inside the call.
 */
#ifndef LVI_FMAT_H
#define LVI_FMAT_H

#include "lvi_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_FMAT_ABI_VERSION    1
#define LVI_FMAT_MAX_POINTS     3072   /* upper bound of max_points (points live in LDS, 16 B each) */
#define LVI_FMAT_MAX_ITERS      4096   /* upper bound of max_iters */

/* lvi_fmat_info.path (whether a model was found: best_iter >= 0) */
#define LVI_FMAT_PATH_KERNEL    1      /* n == 7: the 7-point kernel alone, status all ones */
#define LVI_FMAT_PATH_LMEDS     2      /* 8 <= n < 15 */
#define LVI_FMAT_PATH_RANSAC    3      /* n >= 15 */

typedef struct lvi_fmat lvi_fmat;

typedef struct lvi_fmat_info {
    int32_t path;          /* LVI_FMAT_PATH_* */
    int32_t iters;         /* iterations the walk ran */
    int32_t n_subsets;     /* subsets the sample stream produced (the walk never runs past them) */
    int32_t best_iter;     /* iteration and root of the chosen model; -1 = no model, the status is all zeros
                              (except on the kernel path, whose status is all ones whatever the kernel returns) */
    int32_t best_root;
    int32_t n_inliers;     /* ones in the status */
    double  best_median;   /* LMeDS: the winning median error; otherwise 0 */
    double  F[9];          /* the chosen model, row-major; zeros when none */
    double  stream_us;     /* host time of the sample stream (cv::RNG + getSubset) of this call */
} lvi_fmat_info;

int32_t lvi_fmat_abi_version(void);

/* max_points: largest n of one call (7..LVI_FMAT_MAX_POINTS); max_iters: OpenCV's maxIters
 * (1..LVI_FMAT_MAX_ITERS; the reference's call uses the default, 1000). */
int32_t lvi_fmat_create(int32_t device, int32_t max_points, int32_t max_iters, lvi_fmat **out);
void lvi_fmat_destroy(lvi_fmat *h);

/* checkSubset of the sample stream: 1 (default) = haveCollinearPoints on both point sets,
 * 0 = accept every subset of distinct indices.  DESIGN §11 says why this is a switch. */
int32_t lvi_fmat_set_check_subset(lvi_fmat *h, int32_t mode);

/* pts1_xy, pts2_xy: [n][2] float (un_cur, un_forw).  status_out [n]: 1 = inlier.  info_out may
 * be NULL.  n < 7 or n > max_points: LVI_ERR_INVALID_ARG and nothing is written.  One wait. */
int32_t lvi_fmat_find(lvi_fmat *h, const float *pts1_xy, const float *pts2_xy, int32_t n, double threshold, double confidence,
                      uint8_t *status_out, lvi_fmat_info *info_out);

/* ---- introspection of the last lvi_fmat_find (tests) ---------------------------------------------
 * subsets [cap][7]: the sample stream; nmodels [cap]: candidates of each hypothesis (0..3);
 * F [cap][3][9]: the candidates; score [cap][3]: inlier count (RANSAC) or the median error's f32
 * bit pattern (LMeDS).  Any pointer may be NULL; *n_out = the number of hypotheses (n_subsets). */
int32_t lvi_fmat_trace(lvi_fmat *h, int32_t *subsets, int32_t *nmodels, double *F, int32_t *score, int32_t cap, int32_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* LVI_FMAT_H */
