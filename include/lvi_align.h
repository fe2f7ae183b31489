/* lvi_align.h — the visual-inertial alignment of vins_estimator's initialisation on the GPU: gyro bias, scale, gravity.
 *
 * Replaces tmp_pre_integration and the all_image_frame insert (estimator.cpp:99, :132-135), the erase of the old slide
 * (:1019-1033), the excitation check (:273-300), solveGyroscopeBias, TangentBasis, RefineGravity, LinearAlignment and
 * VisualIMUAlignment (initial/initial_aligment.cpp:3-209) and the tail of Estimator::visualInitialAlign with Utility::g2R
 * (estimator.cpp:450-486).  The contract is DESIGN §31.
 *
 * The handle holds an ordered list of up to caps.max_frames image frames.  A frame is a stamp, R and T (identity and zero until
 * lvi_align_set_pose), an is_key_frame byte and its preintegration: a sample buffer of caps.max_samples and sum_dt, delta_p,
 * delta_q, delta_v, linearized_ba / bg, linearized_acc / gyr and the 15 x 15 jacobian.  THE COVARIANCE OF A FRAME'S
 * PREINTEGRATION IS READ NOWHERE IN THE REFERENCE'S ALIGNMENT AND IS NOT COMPUTED.  The first frame ever added has no
 * preintegration (estimator.cpp:48-50 deletes none for it).  Beside the list there is one pending preintegration,
 * tmp_pre_integration, and the estimator's acc_0 / gyr_0 (on the host: the last sample pushed).
 *
 * All arithmetic is double in the order csrc/lvi_align_math.hpp states, over csrc/lvi_preint_math.hpp, without fused
 * multiply-adds and without matrix instructions: a frame's record is bit for bit the record of an lvi_preint slot fed the
 * same samples and biases, and a solve equals tests/align_ref.py in float64 bit for bit.  The symmetric solve is the
 * restatement's own (an unpivoted L D L' on the band and the border; Eigen's pivoted LDLT is not reproduced).
 *
 * Every entry point checks its arguments before it enqueues anything and leaves all state as it was on an error.  Work is
 * enqueued on the handle's one stream; lvi_align_push_imu and lvi_align_add_frame do not wait for it, every entry point that
 * returns values does.  Exported by liblvi_hip.so only; a separate ABI from lvi_hotpath.h, whose version it does not change.
 */
#ifndef LVI_ALIGN_H
#define LVI_ALIGN_H

#include "lvi_preint.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_ALIGN_ABI_VERSION        1
#define LVI_ALIGN_MAX_FRAMES         256    /* upper bound of caps.max_frames */
#define LVI_ALIGN_SYSTEMS            5      /* LinearAlignment and the four passes of RefineGravity */

/* lvi_align_info.reason */
#define LVI_ALIGN_OK                     0
#define LVI_ALIGN_GRAVITY_NORM           1  /* | |g| - |G| | > 1 after LinearAlignment (:185) */
#define LVI_ALIGN_NEGATIVE_SCALE         2  /* s < 0 after LinearAlignment (:185) */
#define LVI_ALIGN_NEGATIVE_SCALE_REFINED 3  /* s < 0 after RefineGravity (:195) */
#define LVI_ALIGN_SINGULAR               4  /* a pivot that is not finite or not > 0, or fewer equations than unknowns */
#define LVI_ALIGN_TOO_FEW                5  /* fewer than two frames: nothing was done */
/* lvi_align_apply's flags */
#define LVI_ALIGN_APPLY_OPPOSITE         1  /* g2R met a gravity along -z: the rotation by pi about x was taken */

typedef struct lvi_align lvi_align;

typedef struct lvi_align_caps {
    int32_t max_frames;          /* 2..LVI_ALIGN_MAX_FRAMES */
    int32_t max_samples;         /* samples one frame's preintegration can hold, 1..LVI_PREINT_MAX_SAMPLES */
} lvi_align_caps;

typedef struct lvi_align_params {
    double acc_n, gyr_n, acc_w, gyr_w;   /* kept beside the preintegrations as in lvi_preint_params; no covariance reads them */
    double G[3];                 /* only its norm is read (:56, :185) */
    double TIC[3];               /* TIC[0] */
} lvi_align_params;

typedef struct lvi_align_info {
    int32_t ok;                  /* VisualIMUAlignment's boolean */
    int32_t reason;
    int32_t n_state;             /* the length of x: 3 F + 3 after the refinement, 3 F + 4 otherwise */
    int32_t frames;              /* F */
    double delta_bg[3];
    double s;                    /* x(n - 1) / 100 of the last system solved */
    double g_linear[3];          /* g before the refinement */
    double g[3];                 /* g as the reference leaves it: refined when the linear gates passed */
    double min_pivot[6];         /* the smallest pivot of the gyro solve, LinearAlignment and the four passes; 0 when not reached */
} lvi_align_info;

typedef struct lvi_align_frame {
    double stamp;
    double R[9], T[3];
    int32_t is_key_frame, has_preintegration, samples, reserved;
    double sum_dt, delta_p[3], delta_q[4], delta_v[3], linearized_ba[3], linearized_bg[3], linearized_acc[3], linearized_gyr[3];
    double jacobian[225];
} lvi_align_frame;

int32_t lvi_align_abi_version(void);
/* lvi_preint_params_default's values and TIC 0 0 0 */
void lvi_align_params_default(lvi_align_params *p);
/* device memory: (max_frames + 1) slots of 56 max_samples + 2 KB each, and 0.5 MB of systems and pair products sized for
 * LVI_ALIGN_MAX_FRAMES */
int32_t lvi_align_create(int32_t device, const lvi_align_caps *caps, lvi_align **out);
void lvi_align_destroy(lvi_align *h);
int32_t lvi_align_set_params(lvi_align *h, const lvi_align_params *p);
/* clearState (:48-73): no frame, no pending preintegration, no sample seen */
int32_t lvi_align_clear(lvi_align *h);
/* :99 for n samples: dt [n], acc [n][3], gyr [n][3], all finite.  The pending preintegration takes them; before the first
 * frame exists there is none and only acc_0 / gyr_0 move, as in lvi_preint_push with frame 0.  LVI_ERR_CAPACITY when the
 * pending preintegration would exceed caps.max_samples. */
int32_t lvi_align_push_imu(lvi_align *h, int32_t n, const double *dt, const double *acc, const double *gyr);
/* :132-135: a frame with this stamp takes the pending preintegration, and a fresh IntegrationBase{acc_0, gyr_0, Ba, Bg}
 * becomes the pending one.  LVI_ERR_CAPACITY at max_frames; LVI_ERR_INVALID_ARG for a stamp that is not greater than the
 * last; LVI_ERR_STATE when no sample was ever pushed (acc_0 and gyr_0 are not defined). */
int32_t lvi_align_add_frame(lvi_align *h, double stamp, const double *Ba, const double *Bg);
/* :1019-1033: the frames with stamp <= t0 go.  LVI_ERR_STATE if t0 is no frame's stamp.  No sample moves. */
int32_t lvi_align_erase_through(lvi_align *h, double t0);
/* what initialStructure writes from the SFM (:339-410) and the flag of :434.  R and T are taken as they stand: a value that
 * is not finite shows as LVI_ALIGN_SINGULAR in the solve.  LVI_ERR_STATE if stamp is no frame's. */
int32_t lvi_align_set_pose(lvi_align *h, double stamp, const double *R, const double *T, int32_t is_key_frame);
int32_t lvi_align_frames(lvi_align *h, int32_t *count);
/* :273-300: *var.  The reference leaves sum_g uninitialised; here it starts at 0.  A frame whose sum_dt is 0 gives what the
 * division gives.  LVI_ERR_STATE with fewer than two frames. */
int32_t lvi_align_excitation(lvi_align *h, double *var);
/* VisualIMUAlignment (:201-209).  Bgs_inout [11][3] is advanced by delta_bg and every frame's preintegration is
 * repropagated with Ba = 0 and the new Bgs[0], whatever the result (:28-35).  g_out [3] and x_out [info.n_state] as the
 * reference leaves them; zero when the reason is LVI_ALIGN_SINGULAR or _TOO_FEW.  cap: the doubles x_out holds, at least
 * 3 F + 4 (LVI_ERR_CAPACITY).  One upload, one chain of launches, one download, one wait. */
int32_t lvi_align_solve(lvi_align *h, double *Bgs_inout, double *g_out, double *x_out, int32_t cap, lvi_align_info *info);
/* the frame at `index` of the list; dt [cap], acc [cap][3], gyr [cap][3] may each be NULL.  LVI_ERR_CAPACITY when cap is
 * too small for an array that is given. */
int32_t lvi_align_get_frame(lvi_align *h, int32_t index, lvi_align_frame *out, int32_t cap, double *dt, double *acc, double *gyr);
/* the normal equations of the last solve as they were factored: which = 0 LinearAlignment, 1..4 the passes of
 * RefineGravity.  *n its size; A [n][n] dense row-major, b [n], x [n] (the last pass's x has its tail divided by 100), each
 * may be NULL; cap: the doubles A holds (b and x hold n).  LVI_ERR_STATE when the last solve did not build it. */
int32_t lvi_align_last_system(lvi_align *h, int32_t which, int32_t *n, double *A, double *b, double *x, int32_t cap);
/* The tail of visualInitialAlign (:450-486), on the host over csrc/lvi_align_math.hpp; it uses atan2, sin and cos, so it is
 * held to a tolerance, not to bits.  Ps [frame_count + 1][3] and Rs [frame_count + 1][9] hold the frames' T and R on entry
 * (:428-435); Ps[i] = s Ps[i] - Rs[i] TIC - (s Ps[0] - Rs[0] TIC) for i descending, s = x[n_x - 1]; Vs[kv] = key_R[kv]
 * x.segment(3 kv) over the n_key key frames of the list in list order; then g2R, the yaw removed, and g, Ps, Rs, Vs rotated
 * by rot_diff [9] (may be NULL).  FromTwoVectors' branch for nearly opposite vectors chooses an axis by SVD; here the
 * rotation by pi about x is taken and *flags gets LVI_ALIGN_APPLY_OPPOSITE.  The depth rescale, the re-triangulation and
 * the window's repropagate stay with lvi_fman_* and lvi_preint_repropagate. */
int32_t lvi_align_apply(const lvi_align_params *params, int32_t frame_count, double *Ps, double *Rs, double *Vs, const double *x, int32_t n_x, double *g,
                        const double *key_R, int32_t n_key, double *rot_diff, int32_t *flags);

#ifdef __cplusplus
}
#endif
#endif /* LVI_ALIGN_H */
