/* lvi_pgo.h — mapOptimization's factor graph on the GPU: the keyframe pose graph and its optimisation.
 *
 * Replaces addOdomFactor (mapOptimization.cpp:1414-1428), addLoopFactor (:1509-1527), the isam->update calls and the
 * estimate read-back of saveKeyFramesAndFactor (:1546-1599) and the pose source of correctPoses (:1615-1646).  GPS
 * factors (addGPSFactor, :1430-1507) and the covariance that gates them (:1591) operate on this handle through
 * lvi_pgo_gps.h, a separate header with its own version.  GTSAM is not vendored: the conventions are restated from memory
 *  — tangent order rotation then translation, Rot3::RzRyRx(roll, pitch, yaw), right perturbations, factor
 * error = Local(measured, h(x)) whitened by 1 / sqrt(variance).  Parity is with the MINIMISER of that cost
 * (tests/pgo_ref.py), not with iSAM2's iterate after its 2 (or 7) updates.
 * Exported by liblvi_hip.so only (the CPU oracle does not implement it); a separate ABI from lvi_hotpath.h, whose version
 * it does not change.
 *
 * The graph is a chain (prior on key 0, one odometry edge per later key) plus up to max_loops loop edges.  All device
 * arithmetic is double.
 */
#ifndef LVI_PGO_H
#define LVI_PGO_H

#include "lvi_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_PGO_ABI_VERSION     1
#define LVI_PGO_MAX_POSES       65536  /* upper bound of max_poses */
#define LVI_PGO_MAX_LOOPS       64     /* upper bound of max_loops: the loop system (6 x max_loops square) is factored by one workgroup */
#define LVI_PGO_MAX_ITERS       64     /* upper bound of lvi_pgo_params.max_iters */

/* soft status of lvi_pgo_solve (> 0) */
#define LVI_PGO_NOT_CONVERGED   1      /* max_iters Gauss-Newton steps were taken and the last was not below conv_eps */

typedef struct lvi_pgo lvi_pgo;

typedef struct lvi_pgo_params {
    int32_t full_logmap;   /* 1: Local / Retract = Pose3::Logmap / Expmap (GTSAM_POSE3_EXPMAP, the default of recent GTSAM
                              releases); 0: the chart [Rot3::Logmap(R); t] / (Rot3::Expmap(w), v).  Which of the two the
                              reference's GTSAM build uses is not known here */
    int32_t max_iters;     /* Gauss-Newton steps at most (1..LVI_PGO_MAX_ITERS) */
    double  conv_eps;      /* converged when the largest |component| of a step is below this */
} lvi_pgo_params;

typedef struct lvi_pgo_info {
    int32_t iterations;    /* Gauss-Newton steps taken */
    int32_t converged;     /* the last step was below conv_eps */
    double  chi2_before;   /* sum of squared whitened errors at the poses the solve started from */
    double  chi2_after;    /* ... at the poses it left */
    double  max_step;      /* largest |component| of the last step */
} lvi_pgo_info;

int32_t lvi_pgo_abi_version(void);
void lvi_pgo_params_default(lvi_pgo_params *p);      /* full_logmap 1, max_iters 10, conv_eps 1e-10 */

/* max_poses 1..LVI_PGO_MAX_POSES, max_loops 0..LVI_PGO_MAX_LOOPS.  Memory grows with max_poses * (6 max_loops + 6):
 * the right-hand sides of a step (6 max_loops + 1) or of lvi_pgo_gps_marginal_covariance (6 max_loops + 6). */
int32_t lvi_pgo_create(int32_t device, int32_t max_poses, int32_t max_loops, lvi_pgo **out);
void lvi_pgo_destroy(lvi_pgo *g);
int32_t lvi_pgo_clear(lvi_pgo *g);                   /* no poses, no loops; the parameters stay */
int32_t lvi_pgo_set_params(lvi_pgo *g, const lvi_pgo_params *p);
int32_t lvi_pgo_count(lvi_pgo *g, int32_t *n_poses, int32_t *n_loops);

/* addOdomFactor (:1414-1428) and the initialEstimate.insert beside it.  Poses are (roll, pitch, yaw, x, y, z) floats as
 * trans2gtsamPose / pclPointTogtsamPose3 read them.  The first call adds PriorFactor(0, pose_to) with variances
 * (1e-2, 1e-2, pi^2, 1e8, 1e8, 1e8) (:1418-1420; pose_from is ignored and may be NULL); a later call adds
 * BetweenFactor(n - 1, n, poseFrom.between(poseTo)) with variances (1e-6 x3, 1e-4 x3) (:1422-1427).  The measurement is
 * computed here, in double, from the two float poses and kept; pose_to is the new key's initial estimate.  *index_out
 * (may be NULL) = the new key's index.  LVI_ERR_CAPACITY beyond max_poses; nothing changes on an error. */
int32_t lvi_pgo_add_pose(lvi_pgo *g, const float pose_from[6], const float pose_to[6], int32_t *index_out);

/* addLoopFactor (:1509-1527), one queue entry: BetweenFactor(from, to, between) with six equal variances (the float
 * fitness score).  between: row-major 4x4 (rigid).  from == to, an index outside the keys added so far, variance <= 0
 * or not finite: LVI_ERR_INVALID_ARG; more than max_loops: LVI_ERR_CAPACITY.  The arguments are checked before
 * anything is touched and an error leaves all state as it was. */
int32_t lvi_pgo_add_loop(lvi_pgo *g, int32_t from, int32_t to, const double between[16], float variance);

/* isam->update + calculateEstimate (:1546-1566) as the minimiser: undamped Gauss-Newton on SE(3) until the largest
 * step component is below conv_eps, at most max_iters steps.  Every step is an exact solve of the normal equations that
 * uses the graph's structure (chain by block cyclic reduction, loops by a dense Schur system, key 0 by the prior alone:
 * DESIGN §18); no linear algebra runs on the host.  The whole solve is enqueued at once and waited for once; whether a
 * step still has to be taken is decided on the device, and the launches behind a finished solve return at once.
 * Returns LVI_OK, LVI_PGO_NOT_CONVERGED or an error (LVI_ERR_STATE without poses).  info_out may be NULL. */
int32_t lvi_pgo_solve(lvi_pgo *g, lvi_pgo_info *info_out);

/* isamCurrentEstimate.at<Pose3>(i) for i = first .. first + count - 1 (:1567-1599, :1627-1640).  T [count][16]:
 * row-major 4x4 doubles; rpyxyz [count][6]: the float casts of roll = atan2(R21, R22), pitch = atan2(-R20, hypot(R21,
 * R22)), yaw = atan2(R10, R00) and the translation (Rot3::roll / pitch / yaw).  Either may be NULL. */
int32_t lvi_pgo_get_poses(lvi_pgo *g, int32_t first, int32_t count, double *T, float *rpyxyz);

#ifdef __cplusplus
}
#endif
#endif /* LVI_PGO_H */
