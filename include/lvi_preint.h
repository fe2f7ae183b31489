/* lvi_preint.h — the IMU preintegration of vins_estimator's sliding window on the GPU.
 *
 * Replaces Estimator::processIMU (estimator.cpp:82-116), IntegrationBase (factor/integration_base.h:9-158: push_back,
 * propagate, midPointIntegration, repropagate), the repropagate loop of the lidar branch of Estimator::initialStructure
 * (estimator.cpp:215-269) and the preintegration side of both branches of Estimator::slideWindow (:988-1016, :1043-1068).
 * The contract is DESIGN §29.
 *
 * The handle holds LVI_PREINT_SLOTS slots, one for each of pre_integrations[0..WINDOW_SIZE].  A slot is a sample buffer
 * (dt, acc, gyr: the one copy of dt_buf / linear_acceleration_buf / angular_velocity_buf, which the reference keeps twice)
 * and the state of its IntegrationBase.  Beside them it holds one navigation state, Ps / Rs / Vs / Bas / Bgs [j] of the slot
 * being pushed, and the estimator's acc_0, gyr_0 and first_imu (on the host: they are the last sample pushed).
 *
 * One launch runs a list of jobs, one workgroup of 256 threads each: thread r * 15 + c owns element (r, c) of jacobian and
 * covariance; samples are staged LVI_PREINT_CHUNK at a time.  All arithmetic is double in the order
 * csrc/lvi_preint_math.hpp states, without fused multiply-adds and without matrix instructions, so a slot's record depends
 * only on the values it was created with and on its sample sequence: not on how the samples were split into pushes, not on
 * the slot index, not on how many jobs shared the launch, and not on whether it was reached by lvi_preint_push, by the
 * re-push of lvi_preint_slide_new or by lvi_preint_repropagate with the same biases.  All of these are bit-identical, and
 * equal to tests/preint_ref.py in float64.
 *
 * Every entry point checks its arguments before it touches anything and leaves all state as it was on an error.  Work is
 * enqueued on the handle's one stream; lvi_preint_push, _repropagate, _slide_old and _slide_new do not wait for it, every
 * entry point that returns values does.  Exported by liblvi_hip.so only; a separate ABI from lvi_hotpath.h, whose version it
 * does not change.  The record is lvi_win_imu itself: what lvi_preint_get returns goes to lvi_win_add_imu unchanged.
 */
#ifndef LVI_PREINT_H
#define LVI_PREINT_H

#include "lvi_win.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_PREINT_ABI_VERSION       1
#define LVI_PREINT_SLOTS             11     /* WINDOW_SIZE + 1 (parameters.h) */
#define LVI_PREINT_MAX_SAMPLES       8192   /* upper bound of caps.max_samples */
#define LVI_PREINT_CHUNK             16     /* samples one workgroup stages into LDS at a time */

typedef struct lvi_preint lvi_preint;

typedef struct lvi_preint_caps {
    int32_t max_samples;         /* samples one slot can hold, 1..LVI_PREINT_MAX_SAMPLES */
    int32_t reserved;
} lvi_preint_caps;

typedef struct lvi_preint_params {
    double acc_n, gyr_n, acc_w, gyr_w;   /* ACC_N, GYR_N, ACC_W, GYR_W: the noise of integration_base.h:21-27 */
    double G[3];                 /* gravity of the navigation step (estimator.cpp:106-109) and of lvi_preint_evaluate */
} lvi_preint_params;

/* Ps, Rs (row-major 3 x 3), Vs, Bas, Bgs of one window slot */
typedef struct lvi_preint_nav {
    double P[3], R[9], V[3], Ba[3], Bg[3];
} lvi_preint_nav;

int32_t lvi_preint_abi_version(void);
/* acc_n 0.08, gyr_n 0.004, acc_w 4e-5, gyr_w 2e-6, G 0 0 9.8 */
void lvi_preint_params_default(lvi_preint_params *p);
/* device memory: 11 slots of 56 max_samples + 3.8 KB each; pinned: two staging buffers of 56 max_samples bytes */
int32_t lvi_preint_create(int32_t device, const lvi_preint_caps *caps, lvi_preint **out);
void lvi_preint_destroy(lvi_preint *h);
/* setParameter and the noise of :21-27; finite, the four noise values >= 0.  Applies to the samples integrated from now on. */
int32_t lvi_preint_set_params(lvi_preint *h, const lvi_preint_params *p);
/* clearState: no slot exists, first_imu false, the navigation state P 0, R identity, V 0, Ba 0, Bg 0 */
int32_t lvi_preint_clear(lvi_preint *h);
/* The window arrays' entry of the newest slot.  The caller sets it after every solve and BEFORE the slide, as double2vector
 * precedes slideWindow: the slot a slide makes fresh is created with nav.Ba and nav.Bg. */
int32_t lvi_preint_set_nav(lvi_preint *h, const lvi_preint_nav *nav);
int32_t lvi_preint_get_nav(lvi_preint *h, lvi_preint_nav *nav);
/* n calls of processIMU (estimator.cpp:82-116) with this frame_count (0..WINDOW_SIZE): dt [n], acc [n][3], gyr [n][3],
 * all finite.  The first sample ever initialises acc_0 and gyr_0 (:84-89); the slot is created from (acc_0, gyr_0, nav.Ba,
 * nav.Bg) if it does not exist (:91-94); with frame_count != 0 every sample is integrated and steps the navigation state
 * (:95-113); with frame_count == 0 only acc_0 and gyr_0 move.  One upload and one launch; n == 0 does nothing.
 * LVI_ERR_CAPACITY when the slot would exceed caps.max_samples: the reference's buffers grow without bound, but past
 * sum_dt > 10 it drops the factor anyway (:740), so a slot sized for ten seconds of samples loses nothing. */
int32_t lvi_preint_push(lvi_preint *h, int32_t frame_count, int32_t n, const double *dt, const double *acc, const double *gyr);
/* IntegrationBase::repropagate (:38-52) of every slot whose bit is set in mask (bits 0..10), with Bas [11][3] and
 * Bgs [11][3] indexed by slot: one launch for all of them.  A slot in the mask that does not exist: LVI_ERR_STATE. */
int32_t lvi_preint_repropagate(lvi_preint *h, uint32_t mask, const double *Bas, const double *Bgs);
/* estimator.cpp:988-1016: slot i takes slot i + 1 and slot 10 becomes a fresh IntegrationBase{acc_0, gyr_0, nav.Ba, nav.Bg}
 * without samples.  No sample moves. */
int32_t lvi_preint_slide_old(lvi_preint *h);
/* :1043-1068: slot 10's samples are pushed onto slot 9, which continues from its own state with its own linearized_ba / bg
 * and its own acc_0; then slot 10 is made fresh.  LVI_ERR_STATE unless slots 9 and 10 exist; LVI_ERR_CAPACITY, and nothing
 * changes, when slot 9 has too little room. */
int32_t lvi_preint_slide_new(lvi_preint *h);
/* the record lvi_win_add_imu takes, with ids 0; *samples: the slot's sample count.  Either may be NULL.  LVI_ERR_STATE
 * when the slot does not exist. */
int32_t lvi_preint_get(lvi_preint *h, int32_t slot, lvi_win_imu *out, int32_t *samples);
/* the slot's buffers: dt [cap], acc [cap][3], gyr [cap][3], each may be NULL; LVI_ERR_CAPACITY when cap is too small for
 * an array that is given */
int32_t lvi_preint_get_samples(lvi_preint *h, int32_t slot, int32_t cap, int32_t *count, double *dt, double *acc, double *gyr);
/* IMUFactor::Evaluate (imu_factor.h:18-178) of the slot's record at these blocks with sqrt_info applied and G of the
 * parameters, computed on the host with csrc/lvi_imu_math.hpp: residual [15] and jacobians 15 x 7, 15 x 9, 15 x 7, 15 x 9 in
 * turn, row-major, the seventh column of a pose block zero: the layout of VinsMarginalizer::imuResidual / imuJacobians.
 * jacobians may be NULL.  LVI_ERR_STATE when the slot does not exist or its covariance is not positive definite. */
int32_t lvi_preint_evaluate(lvi_preint *h, int32_t slot, const double *pose_i, const double *sb_i, const double *pose_j, const double *sb_j,
                            double *residual, double *jacobians);

#ifdef __cplusplus
}
#endif
#endif /* LVI_PREINT_H */
