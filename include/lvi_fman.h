/* lvi_fman.h — vins_estimator's FeatureManager on the GPU: the feature table every image passes through.
 *
 * Replaces feature_manager.{h,cpp}: addFeatureCheckParallax (:45-106) with compensatedParallax2 (:381-414), getCorresponding
 * (:129-148), setDepth / removeFailures / clearDepth / getDepthVector (:150-211), triangulate (:213-268), removeBackShiftDepth /
 * removeBack / removeFront (:285-379), and the two loops of Estimator::optimization that turn the table into projection
 * factors (estimator.cpp:745-789 and :849-889).  The contract is DESIGN §26.
 *
 * The table lives on the device in the reference's LIST ORDER (std::list<FeaturePerId>), which every operation preserves;
 * only the observations of the new frame go up per image.  Structural work (id match, prefix scan, stable compaction) is one
 * launch of one workgroup over the whole table, which is where the bound of LVI_FMAN_MAX_FEATURES comes from; no workgroup
 * ever waits for another.  All values are doubles and all arithmetic is double, in the order csrc/lvi_fman_math.hpp states,
 * without fused multiply-adds: everything but the triangulated depth is reproducible bit for bit (tests/fman_ref.py).
 *
 * Every entry point checks its arguments before it touches anything, leaves all state as it was on an error, enqueues on the
 * handle's one stream and waits at most once.  Exported by liblvi_hip.so only; a separate ABI from lvi_hotpath.h, whose
 * version it does not change.  The projection record is lvi_marg_projection itself.
 */
#ifndef LVI_FMAN_H
#define LVI_FMAN_H

#include "lvi_marg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_FMAN_ABI_VERSION         1
#define LVI_FMAN_MAX_FEATURES        4096   /* upper bound of max_features: what one workgroup scans in four rounds */
#define LVI_FMAN_WINDOW              10     /* WINDOW_SIZE (parameters.h), compile-time as there */
#define LVI_FMAN_MAX_OBS             11     /* observations of one feature: frames 0..WINDOW_SIZE */
#define LVI_FMAN_MAX_SWEEPS          30     /* sweep bound of the triangulation's Jacobi SVD */

/* mode of lvi_fman_projections */
#define LVI_FMAN_MODE_WINDOW         0      /* estimator.cpp:745-789: every eligible feature */
#define LVI_FMAN_MODE_MARG_OLD       1      /* :849-889: feature_index advances for every eligible feature, records for start_frame == 0 only */

typedef struct lvi_fman lvi_fman;

typedef struct lvi_fman_params {
    double init_depth;           /* INIT_DEPTH = 5.0 (parameters.cpp:116) */
    double min_parallax;         /* MIN_PARALLAX = keyframe_parallax / FOCAL_LENGTH = 10 / 460 */
} lvi_fman_params;

/* FeaturePerFrame (feature_manager.h:16-42): the fields that are ever read */
typedef struct lvi_fman_obs {
    double point[3];
    double uv[2];
    double velocity[2];
    double depth;                /* lidar depth of the observation; <= 0: none (-1 from the tracker node) */
    double cur_td;
} lvi_fman_obs;

/* FeaturePerId (feature_manager.h:44-77) */
typedef struct lvi_fman_feature {
    int32_t feature_id;
    int32_t start_frame;
    int32_t n_obs;               /* feature_per_frame.size() */
    int32_t lidar_depth_flag;
    int32_t solve_flag;          /* 0 not solved yet, 1 solved, 2 failed */
    int32_t reserved;
    double  estimated_depth;
    lvi_fman_obs obs[LVI_FMAN_MAX_OBS];
} lvi_fman_feature;

typedef struct lvi_fman_frame_info {
    int32_t last_track_num;      /* :51, :70 */
    int32_t parallax_num;        /* :92; 0 when one of the two early returns of :83-84 was taken */
    int32_t keyframe;            /* the returned bool: 1 MARGIN_OLD, 0 MARGIN_SECOND_NEW */
    int32_t added;               /* features appended by this frame */
    double  parallax_sum;        /* :91, summed in list order */
} lvi_fman_frame_info;

typedef struct lvi_fman_tri_info {
    int32_t triangulated;        /* features that passed the skip rule of :218-222 */
    int32_t non_finite;          /* ... whose depth is NaN or infinite (stored as it is) */
    int32_t negative;            /* ... whose depth was < 0 and became init_depth */
    int32_t max_sweeps;          /* the most sweeps one SVD took */
} lvi_fman_tri_info;

/* block-id bases of lvi_fman_projections: pose_i = pose + imu_i, pose_j = pose + imu_j, feature = feature + feature_index;
 * td == -1: ProjectionFactor records (ESTIMATE_TD off) */
typedef struct lvi_fman_ids {
    int32_t pose, ex, td, feature;
} lvi_fman_ids;

int32_t lvi_fman_abi_version(void);
/* init_depth 5.0, min_parallax 10 / 460 */
void lvi_fman_params_default(lvi_fman_params *p);

/* max_features 1..LVI_FMAN_MAX_FEATURES.  Device memory: two tables of 824 bytes per feature (a compaction writes the other
 * one), 1.4 KB per feature for the records and the downloads, and 272 KB for the ids and observations of one frame. */
int32_t lvi_fman_create(int32_t device, int32_t max_features, lvi_fman **out);
void lvi_fman_destroy(lvi_fman *f);
/* init_depth finite and > 0, min_parallax finite */
int32_t lvi_fman_set_params(lvi_fman *f, const lvi_fman_params *p);
/* clearState (:23-26); the parameters stay */
int32_t lvi_fman_clear(lvi_fman *f);
/* feature.size() and getFeatureCount() (:28-42): used_num >= 2 && start_frame < WINDOW_SIZE - 2.  Either may be NULL.  Both
 * are kept on the host from the last operation's one download: nothing is enqueued. */
int32_t lvi_fman_count(lvi_fman *f, int32_t *table_size, int32_t *feature_count);

/* addFeatureCheckParallax (:45-106).  frame_count 0..WINDOW_SIZE; n 0..LVI_FMAN_MAX_FEATURES; ids [n] strictly ascending (the
 * reference iterates a std::map), anything else LVI_ERR_INVALID_ARG; obs [n][8]: x y z u v vx vy depth, the tracker node's
 * message.  A known id gets the observation appended, counts towards last_track_num and, when it brings the first lidar depth
 * (:74-79), sets estimated_depth, lidar_depth_flag and observation 0's depth.  Unknown ids are appended in id order with the
 * constructor's depth rule (feature_manager.h:60-74).  More than max_features features: LVI_ERR_CAPACITY; a known feature that
 * already holds LVI_FMAN_MAX_OBS observations: LVI_ERR_STATE; both with nothing changed.  info_out may be NULL. */
int32_t lvi_fman_add_frame(lvi_fman *f, int32_t frame_count, int32_t n, const int32_t *ids, const double *obs, double td, lvi_fman_frame_info *info_out);

/* triangulate (:213-268) with Ps [11][3], Rs [11][9] row-major, tic [3], ric [9].  The skip rule first (used_num >= 2 &&
 * start_frame < WINDOW_SIZE - 2, and estimated_depth > 0 is kept); then the 2k x 4 matrix from point.normalized(), its right
 * singular vector of the smallest singular value by a one-sided Jacobi SVD on the matrix itself (csrc/lvi_fman_math.hpp: fixed
 * sweep order, stated stop rule), depth = V[2] / V[3], depth < 0 -> init_depth.  One lane per feature and no cross-lane sums: the
 * result does not depend on the feature's slot nor on the run.  A non-finite depth is stored as IEEE gives it.  info_out may be NULL. */
int32_t lvi_fman_triangulate(lvi_fman *f, const double *Ps, const double *Rs, const double *tic, const double *ric, lvi_fman_tri_info *info_out);

/* getDepthVector (:194-211): 1 / estimated_depth, or 1 / init_depth where estimated_depth is not > 0.  cap: the room of dep
 * (may be NULL); *count = getFeatureCount() */
int32_t lvi_fman_get_depth_vector(lvi_fman *f, int32_t cap, int32_t *count, double *dep);
/* setDepth (:150-168): estimated_depth = 1 / x[feature_index], solve_flag 2 where that is < 0, else 1.  n must be
 * getFeatureCount() */
int32_t lvi_fman_set_depth(lvi_fman *f, int32_t n, const double *x);
/* clearDepth (:181-192): the same assignment, lidar_depth_flag = false, solve_flag untouched */
int32_t lvi_fman_clear_depth(lvi_fman *f, int32_t n, const double *x);
/* removeFailures (:170-179): features with solve_flag == 2 leave the table */
int32_t lvi_fman_remove_failures(lvi_fman *f);

/* removeBackShiftDepth (:285-339): marg_R, new_R [9] row-major, marg_P, new_P [3].  start_frame != 0: decremented.  Otherwise
 * observation 0 is erased; fewer than 2 left: the feature is erased; else estimated_depth becomes the new first observation's
 * lidar depth (flag set), or dep_j > 0 (flag cleared), or init_depth (flag cleared) */
int32_t lvi_fman_remove_back_shift_depth(lvi_fman *f, const double *marg_R, const double *marg_P, const double *new_R, const double *new_P);
/* removeBack (:341-357): the same shift without depths; a feature is erased when no observation is left */
int32_t lvi_fman_remove_back(lvi_fman *f);
/* removeFront (:359-379), frame_count 1..WINDOW_SIZE (the reference passes WINDOW_SIZE): start_frame == frame_count is
 * decremented; otherwise, unless endFrame() < frame_count - 1, observation WINDOW_SIZE - 1 - start_frame is erased, and the
 * feature with it when it was the last.  An index outside the feature's observations (undefined in the reference, possible
 * only for frame_count < WINDOW_SIZE) leaves the feature as it is. */
int32_t lvi_fman_remove_front(lvi_fman *f, int32_t frame_count);

/* getCorresponding (:129-148), 0 <= frame_l, frame_r <= WINDOW_SIZE: pairs [count][6] = point of frame_l, point of frame_r,
 * in list order.  cap: the room of pairs (may be NULL) */
int32_t lvi_fman_corresponding(lvi_fman *f, int32_t frame_l, int32_t frame_r, int32_t cap, int32_t *count, double *pairs);

/* The projection factors of Estimator::optimization in the reference's order, from a device-side prefix sum and with one
 * download.  records [*count] (cap: their room); per eligible feature, in feature_index order, inv_dep [*n_features] as
 * getDepthVector gives it and lidar_flags [*n_features] (cap_features: their room).  Every array may be NULL; one that is given
 * and too short: LVI_ERR_CAPACITY. */
int32_t lvi_fman_projections(lvi_fman *f, int32_t mode, const lvi_fman_ids *ids, int32_t cap, int32_t *count, lvi_marg_projection *records,
                             int32_t cap_features, int32_t *n_features, double *inv_dep, int32_t *lidar_flags);

/* the whole table in list order, for tests and the host mirror.  cap: the room of features (may be NULL) */
int32_t lvi_fman_download(lvi_fman *f, int32_t cap, int32_t *count, lvi_fman_feature *features);

#ifdef __cplusplus
}
#endif
#endif /* LVI_FMAN_H */
