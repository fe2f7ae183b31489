/* lvi_loop.h — mapOptimization's loop-closure registration on the GPU: the two submaps and the ICP between them.
 *
 * Restates performLoopClosure (mapOptimization.cpp:549-628) up to the constraint: loopFindNearKeyframes (:719-741: corner_k
 * then surf_k per key through the key's pose, then one VoxelGrid) for the current key alone (source) and for the keys
 * pre - search_num .. pre + search_num clipped to the store (target), the 300 / 1000 point gates, and
 * pcl::IterativeClosestPoint as the project restates it (tests/loop_ref.py; DESIGN §13 — parity is against that
 * restatement, not against PCL).  The clouds come from the device keyframe store of an lvi_lidar handle: nothing
 * travels through the host but the two key indices and the result.  Applying the constraint (addLoopFactor, iSAM2,
 * correctPoses) is the caller's.
 *
 * Exported by liblvi_hip.so only (the CPU oracle does not implement it); a separate ABI from lvi_hotpath.h, whose
 * version it does not change.
 *
 * Arena.  lvi_loop_reserve creates, on first use, the two fused clouds, two VoxelGrid plans, the aligned source, the
 * nearest-neighbour grid and the reduction partials, apart from the local map's and the global map's buffers: a handle
 * that never calls it allocates nothing more, and nothing is allocated after it.
 *
 * Streams.  lvi_loop_start enqueues the whole job — fuses, filters, index, every ICP iteration, the fitness pass — on
 * a stream of its own and returns without waiting: the reference runs it on a thread of its own, and the scan path
 * must not wait for it.  That stream first waits for everything enqueued on the handle's main stream so far.  Poses
 * are read from the store when the job is enqueued.  The host waits once per job, in lvi_loop_result.
 *
 * Concurrency (the global map's rule).  lvi_loop_result and lvi_loop_fetch may run on another host thread concurrently
 * with any other call on the handle, except lvi_loop_start, lvi_loop_debug_step, lvi_loop_reserve, lvi_loop_release,
 * lvi_keyframes_clear and lvi_lidar_destroy.  Those are called from the thread that owns the handle (or under its
 * lock); reserve, release, clear and destroy wait for a job in flight.  result and fetch are called from one thread at
 * a time.  A loop job and a global-map build may be in flight together.  Errors are reported per thread
 * (lvi_last_error) and leave all state as it was; the job's launches are not profiled (lvi_prof_*).
 */
#ifndef LVI_LOOP_H
#define LVI_LOOP_H

#include "lvi_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_LOOP_ABI_VERSION 1
#define LVI_LOOP_MAX_POINTS  (1 << 24)   /* largest reservation of either fused cloud */
#define LVI_LOOP_MAX_ITERS   1000        /* largest max_iters */
#define LVI_LOOP_N_SUMS      17          /* count, sum p (3), sum q (3), sum p q^T (9, row-major: p row, q column), sum d2 */

enum { LVI_LOOP_SOURCE = 0, LVI_LOOP_TARGET = 1, LVI_LOOP_ALIGNED = 2 };
/* status of a job */
enum {
    LVI_LOOP_OK = 0,
    LVI_LOOP_TOO_FEW_POINTS = 1,         /* filtered source < min_source or filtered target < min_target: no ICP ran */
    LVI_LOOP_NO_CORRESPONDENCES = 2      /* an iteration kept fewer than 3 pairs: not converged */
};
/* DefaultConvergenceCriteria's states */
enum {
    LVI_LOOP_CONV_NOT_CONVERGED = 0,
    LVI_LOOP_CONV_ITERATIONS = 1,
    LVI_LOOP_CONV_TRANSFORM = 2,
    LVI_LOOP_CONV_ABS_MSE = 3,
    LVI_LOOP_CONV_REL_MSE = 4,
    LVI_LOOP_CONV_NO_CORRESPONDENCES = 5
};

typedef struct lvi_loop_params {
    int32_t search_num;                  /* historyKeyframeSearchNum (25): target = keys pre - n .. pre + n */
    float leaf;                          /* mappingSurfLeafSize (0.4): both submaps' VoxelGrid; 0 = no filter */
    float max_corr_dist;                 /* setMaxCorrespondenceDistance(2 * historyKeyframeSearchRadius) */
    int32_t max_iters;                   /* setMaximumIterations(100), 1..LVI_LOOP_MAX_ITERS */
    double transformation_epsilon;       /* setTransformationEpsilon(1e-6) */
    double fitness_epsilon;              /* setEuclideanFitnessEpsilon(1e-6) */
    int32_t min_source;                  /* 300 */
    int32_t min_target;                  /* 1000 */
    /* the one place where the recollection of PCL is uncertain.  1 (default): every iteration transforms the already
     * transformed source by that iteration's step, in f32, as icp.hpp's transformCloud(*input_transformed,
     * *input_transformed, transformation_) does; 0: every iteration transforms the original source by the composed
     * final transformation.  Equal in exact arithmetic. */
    int32_t incremental_cloud;
} lvi_loop_params;

typedef struct lvi_loop_info {
    int32_t status;                      /* LVI_LOOP_OK / _TOO_FEW_POINTS / _NO_CORRESPONDENCES */
    int32_t n_source, n_target;          /* filtered sizes */
    int32_t n_source_fused, n_target_fused;
    int32_t overflow_source, overflow_target;   /* PCL's "leaf size too small" rule fired: the submap is the fused cloud */
    int32_t iterations;                  /* nr_iterations_ */
    int32_t converged;                   /* hasConverged() */
    int32_t convergence_state;           /* LVI_LOOP_CONV_* */
    int32_t n_corr;                      /* pairs kept by the last correspondence pass */
    int32_t key_cur, key_pre;
    float transformation[16];            /* getFinalTransformation(), row-major */
    double fitness;                      /* getFitnessScore(): mean squared NN distance of every aligned source point */
    double mse;                          /* mean kept squared distance of the last pass */
} lvi_loop_info;

int32_t lvi_loop_abi_version(void);
void lvi_loop_params_default(lvi_loop_params *p);

/* the arena for fused submaps of up to max_source_points / max_target_points (1..LVI_LOOP_MAX_POINTS each); a
 * reservation not larger than the current one in both is a no-op, a larger one replaces it (waits for a job in flight;
 * the last result is lost) */
int32_t lvi_loop_reserve(lvi_lidar *h, int32_t max_source_points, int32_t max_target_points);
int32_t lvi_loop_release(lvi_lidar *h);
int32_t lvi_loop_arena_bytes(lvi_lidar *h, int64_t *bytes);

/* enqueue the job for (key_cur, key_pre).  A key out of range, bad parameters: LVI_ERR_INVALID_ARG.  No reservation:
 * LVI_ERR_STATE.  A fused submap above its reservation: LVI_ERR_CAPACITY.  Every error leaves all state as it was (the
 * previous job's result stays readable).  Waits only for a previous job still in flight. */
int32_t lvi_loop_start(lvi_lidar *h, int32_t key_cur, int32_t key_pre, const lvi_loop_params *params);
/* waits for the last job (its stream only); LVI_ERR_STATE before the first job */
int32_t lvi_loop_result(lvi_lidar *h, lvi_loop_info *info);
/* points [first, first + count) of the filtered source, the filtered target or the aligned source (the source under the
 * final transformation) of the last job (implies lvi_loop_result).  The range must lie in the cloud. */
int32_t lvi_loop_fetch(lvi_lidar *h, int32_t what, int32_t first, int32_t count, lvi_pt *out);
/* tests: one correspondence pass of the last job's clouds with the source under T (row-major 4x4, f32:
 * ((m0 x + m1 y) + m2 z) + m3 per row) and the last job's max_corr_dist.  nn_idx / nn_sqd [n_source]: the nearest
 * target point and its squared f32 distance ((dx dx + dy dy) + dz dz), -1 / +inf where none lies within the cut.
 * sums [LVI_LOOP_N_SUMS]: the reduction over the kept pairs.  Changes nothing lvi_loop_result or lvi_loop_fetch
 * return.  Same thread rule as lvi_loop_start. */
int32_t lvi_loop_debug_step(lvi_lidar *h, const float *T, int32_t *nn_idx, float *nn_sqd, double *sums);

#ifdef __cplusplus
}
#endif
#endif /* LVI_LOOP_H */
