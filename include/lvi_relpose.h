/* lvi_relpose.h — the initial two-view pose of vins_estimator's visual initialisation on the GPU.
 *
 * Replaces MotionEstimator::solveRelativeRT (initial/solve_5pts.cpp:193-227: cv::findFundamentalMat(FM_RANSAC) followed by
 * cv::recoverPose with the identity camera matrix) and the frame loop of Estimator::relativePose (estimator.cpp:493-522).
 * The contract is DESIGN §30; parity is against tests/relpose_ref.py, a restatement of OpenCV 4.5.x decomposeEssentialMat,
 * recoverPose and triangulatePoints with an SVD of its own, not against OpenCV itself.
 *
 * lvi_relpose_recover is cv::recoverPose: E is decomposed into the four candidates [R1|t], [R2|t], [R1|-t], [R2|-t], every
 * correspondence is triangulated under each of them (4 n null vectors of 4 x 4 matrices, one lane each), the cheirality
 * and distance masks are applied and counted, and the first candidate whose count is >= the three others is chosen.  All
 * arithmetic is double in the order csrc/lvi_relpose_math.hpp states, without fused multiply-adds and without matrix
 * instructions: every field of the result equals tests/relpose_ref.py bit for bit, and a point's mask bits do not depend
 * on where in the set it stands or on what stands beside it.
 *
 * Every entry point checks its arguments before anything is enqueued and leaves all state as it was on an error.
 * Exported by liblvi_hip.so only; a separate ABI from lvi_hotpath.h, whose version it does not change.
 */
#ifndef LVI_RELPOSE_H
#define LVI_RELPOSE_H

#include "lvi_fmat.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_RELPOSE_ABI_VERSION      1
#define LVI_RELPOSE_MIN_POINTS       15     /* solve_5pts.cpp:195: corres.size() >= 15; lower bound of max_points */
#define LVI_RELPOSE_MIN_INLIERS      12     /* :221: inlier_cnt > 12 */
#define LVI_RELPOSE_CHUNK            64     /* points of one workgroup of relpose_cheirality: one wavefront */

/* lvi_relpose_pose.flags, lvi_relpose_result.flags */
#define LVI_RELPOSE_DEGENERATE       1      /* E has a non-finite entry or a second singular value of exactly 0: R = I, t = 0, all counts 0 */
#define LVI_RELPOSE_NO_MODEL         2      /* lvi_fmat_find found no model (info.best_iter < 0): recover was skipped */
#define LVI_RELPOSE_TOO_FEW          4      /* n < 15 (:195): nothing ran */

typedef struct lvi_relpose lvi_relpose;

typedef struct lvi_relpose_params {
    double threshold;            /* findFundamentalMat's ransacReprojThreshold, :204 */
    double confidence;           /* its confidence */
    double distance_thresh;      /* recoverPose's dist of lvi_relpose_solve */
} lvi_relpose_params;

/* cv::recoverPose's outputs and what it counted */
typedef struct lvi_relpose_pose {
    double  R[9];                /* row-major */
    double  t[3];
    double  sv[3];               /* the singular values of E, descending; zeros when degenerate */
    int32_t good[4];             /* the counts of [R1|t], [R2|t], [R1|-t], [R2|-t] */
    int32_t chosen;              /* 0..3 */
    int32_t n_inliers;           /* good[chosen] */
    int32_t flags;               /* LVI_RELPOSE_DEGENERATE */
    int32_t sweeps;              /* Jacobi sweeps of the decomposition */
} lvi_relpose_pose;

/* MotionEstimator::solveRelativeRT */
typedef struct lvi_relpose_result {
    double  Rotation[9];         /* R' (:219), row-major; identity when recover did not run */
    double  Translation[3];      /* -R' t (:220) */
    double  average_parallax;    /* estimator.cpp:502-512 on the doubles of the pairs; 0 when n == 0 */
    int32_t ok;                  /* n >= 15 and inlier_cnt > 12 */
    int32_t flags;               /* LVI_RELPOSE_* */
    lvi_relpose_pose pose;       /* zeros when recover did not run */
    lvi_fmat_info info;          /* of lvi_fmat_find; zeros when n < 15 */
} lvi_relpose_result;

int32_t lvi_relpose_abi_version(void);
/* threshold 0.3 / 460, confidence 0.99, distance_thresh 50 */
void lvi_relpose_params_default(lvi_relpose_params *p);
/* max_points: largest n of one call (LVI_RELPOSE_MIN_POINTS..LVI_FMAT_MAX_POINTS); max_iters: findFundamentalMat's maxIters
 * (1..LVI_FMAT_MAX_ITERS; :204 uses the default, 1000).  The handle owns an lvi_fmat of the same size. */
int32_t lvi_relpose_create(int32_t device, int32_t max_points, int32_t max_iters, lvi_relpose **out);
void lvi_relpose_destroy(lvi_relpose *h);
/* finite, threshold > 0, 0 < confidence < 1, distance_thresh > 0 */
int32_t lvi_relpose_set_params(lvi_relpose *h, const lvi_relpose_params *p);
/* cv::recoverPose(E, pts1, pts2, I, R, t, mask) (five-point.cpp; the copy at solve_5pts.cpp:30-182).  E [9] row-major;
 * pts1_xy, pts2_xy [n][2] float; n 1..max_points; mask_inout [n]: non-zero = use the point, NULL = all ones and nothing
 * is written back, otherwise it receives the chosen candidate's mask as 0 / 1; distance_thresh finite and > 0.  One
 * upload, two launches, one download, one wait. */
int32_t lvi_relpose_recover(lvi_relpose *h, const double *E, const float *pts1_xy, const float *pts2_xy, int32_t n, uint8_t *mask_inout,
                            double distance_thresh, lvi_relpose_pose *pose);
/* solveRelativeRT on one getCorresponding result: pairs [n][6] (first x y z, second x y z; lvi_fman_corresponding's
 * layout), n 0..max_points.  x and y of both are rounded to float (cv::Point2f, :200-201), lvi_fmat_find runs with the
 * handle's threshold and confidence, then lvi_relpose_recover with its status and info.F.  status_out [n] may be NULL:
 * the status of lvi_fmat_find.  n < 15 and a missing model are not errors: ok = 0 and a flag.  Waits twice. */
int32_t lvi_relpose_solve(lvi_relpose *h, const double *pairs, int32_t n, lvi_relpose_result *result, uint8_t *status_out);
/* average_parallax of estimator.cpp:502-512 over pairs [n][6]: the sum of sqrt(dx dx + dy dy) in list order on the doubles,
 * then 1.0 * sum / n; computed on the host (a sequential sum over pairs that are in host memory).  0 when n < 1 or pairs is NULL. */
double lvi_relpose_average_parallax(const double *pairs, int32_t n);
/* the last lvi_relpose_recover that succeeded (tests): cand [4][12], R row-major then t of each candidate; masks [4][cap]
 * (row stride cap); either may be NULL.  *n_out: its n.  LVI_ERR_STATE when there was none, LVI_ERR_CAPACITY when cap < n. */
int32_t lvi_relpose_last(lvi_relpose *h, double *cand, uint8_t *masks, int32_t cap, int32_t *n_out);
/* the owned lvi_fmat, for lvi_fmat_trace after lvi_relpose_solve (tests) and lvi_fmat_set_check_subset; the handle keeps owning it */
lvi_fmat *lvi_relpose_fmat(lvi_relpose *h);

#ifdef __cplusplus
}
#endif
#endif /* LVI_RELPOSE_H */
