/* lvi_win.h — the solve of vins_estimator's sliding window on the GPU: the first half of Estimator::optimization.
 *
 * Replaces estimator.cpp:696-811: the problem build (:698-789), ceres::Solve with the options of :792-805 (DENSE_SCHUR,
 * DOGLEG, max_num_iterations, max_solver_time_in_seconds) and the write-back (double2vector's input).  Evaluated on the
 * device: ProjectionFactor / ProjectionTdFactor with their loss (csrc/lvi_marg_math.hpp), IMUFactor::Evaluate
 * (imu_factor.h:18-178, integration_base.h:160-186; csrc/lvi_imu_math.hpp) and the previous marginalisation as a
 * MarginalizationFactor (marginalization_factor.cpp:332-380).  The contract is DESIGN §22.
 *
 * Ceres is not part of this repository: the trust-region loop and its TRADITIONAL_DOGLEG strategy are pinned as the
 * algorithm tests/win_ref.py states, not as Ceres' iterates.  Every constant of that loop that was restated from recall is
 * a field of lvi_win_params (DESIGN §22 lists them), so that it can be corrected without a rebuild.
 *
 * Exported by liblvi_hip.so only; a separate ABI from lvi_hotpath.h and lvi_marg.h, whose versions it does not change.
 * All arithmetic is double.  Parameter blocks are named by caller-chosen int32 ids, as in lvi_marg.h, and the projection
 * record is lvi_marg_projection itself: the records built for the solve go to lvi_marg_add_projection unchanged.
 */
#ifndef LVI_WIN_H
#define LVI_WIN_H

#include "lvi_marg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_WIN_ABI_VERSION          1
#define LVI_WIN_MAX_BLOCKS           4096   /* upper bound of caps.max_blocks */
#define LVI_WIN_MAX_PROJECTIONS      8192   /* ... of caps.max_projections */
#define LVI_WIN_MAX_ELIMINATED       2048   /* ... of caps.max_eliminated */
#define LVI_WIN_MAX_IMU              16     /* ... of caps.max_imu */
#define LVI_WIN_MAX_PRIOR_ROWS       256    /* ... of caps.max_prior_rows */
#define LVI_WIN_MAX_DIM              256    /* ... of caps.max_dim, the reduced system: 16 frames x 15 + 6 + 1 = 247 */
#define LVI_WIN_MAX_BLOCK_SIZE       16
#define LVI_WIN_MAX_ITERATIONS       64     /* upper bound of params.max_iterations */
#define LVI_WIN_SHARE                128    /* projection factors one workgroup accumulates before its partial is written */
#define LVI_WIN_CHOL_BLOCK           32     /* the panel width of the blocked Cholesky */

/* flags of lvi_win_set_block */
#define LVI_WIN_CONSTANT             1      /* SetParameterBlockConstant (:715, :775-776, :784-785): no column anywhere */
#define LVI_WIN_ELIMINATED           2      /* size 1, named only in the feature slot of projection records: eliminated by the
                                               Schur complement, no column in the reduced system */

/* soft status of lvi_win_solve (> 0) */
#define LVI_WIN_NOT_FINITE           1      /* a non-finite cost or system at the declared values (inv_dep == 0): the blocks keep them */
#define LVI_WIN_BAD_COVARIANCE       2      /* the covariance of an IMU record is not positive definite: the blocks keep their values */

/* lvi_win_info.termination */
#define LVI_WIN_TERM_NONE            0
#define LVI_WIN_TERM_FUNCTION        1      /* |cost change| <= function_tolerance x cost */
#define LVI_WIN_TERM_GRADIENT        2      /* max |gradient| <= gradient_tolerance */
#define LVI_WIN_TERM_PARAMETER       3      /* |step| <= parameter_tolerance (|x| + parameter_tolerance) */
#define LVI_WIN_TERM_ITERATIONS      4      /* max_iterations reached */
#define LVI_WIN_TERM_TIME            5      /* max_time_s passed */
#define LVI_WIN_TERM_RADIUS          6      /* the radius fell below min_radius */
#define LVI_WIN_TERM_INVALID_STEPS   7      /* max_invalid_steps consecutive steps without a positive model cost change, or no
                                               factorisation up to max_mu */

/* lvi_win_iteration.step_kind */
#define LVI_WIN_STEP_NONE            0
#define LVI_WIN_STEP_GAUSS_NEWTON    1      /* the Gauss-Newton step lies inside the radius */
#define LVI_WIN_STEP_CAUCHY          2      /* the Cauchy point lies outside: the gradient step cut at the radius */
#define LVI_WIN_STEP_INTERPOLATED    3      /* the point of the leg between them that meets the radius */

typedef struct lvi_win lvi_win;

typedef struct lvi_win_caps {
    int32_t max_blocks;          /* parameter blocks declared between two lvi_win_begin */
    int32_t max_projections;
    int32_t max_eliminated;      /* blocks flagged LVI_WIN_ELIMINATED */
    int32_t max_imu;
    int32_t max_prior_rows;      /* n of the prior */
    int32_t max_dim;             /* local size of all free blocks that are not eliminated */
} lvi_win_caps;

/* R: restated from recall of ceres-solver's defaults (Solver::Options, DoglegStrategy); see DESIGN §22 */
typedef struct lvi_win_params {
    int32_t loss_type;           /* LVI_MARG_LOSS_* of the projection factors (estimator.cpp:701) */
    int32_t max_iterations;      /* NUM_ITERATIONS (:796), 0..LVI_WIN_MAX_ITERATIONS */
    int32_t jacobi_scaling;      /* R: 1 */
    int32_t max_invalid_steps;   /* R: 5, max_num_consecutive_invalid_steps */
    double  loss_a, sqrt_info, tr_over_row, half_row;   /* as lvi_marg_params */
    double  G[3];                /* gravity (parameters.h G; 0 0 9.8 before the initialisation sets it) */
    double  max_time_s;          /* max_solver_time_in_seconds (:800-803), checked on the host between iterations; 0: none */
    double  initial_radius;      /* R: 1e4 */
    double  max_radius;          /* R: 1e16 */
    double  min_radius;          /* R: 1e-32 */
    double  min_relative_decrease;   /* R: 1e-3 */
    double  function_tolerance;  /* R: 1e-6 */
    double  gradient_tolerance;  /* R: 1e-10 */
    double  parameter_tolerance; /* R: 1e-8 */
    double  initial_mu;          /* R: 1e-8 (= min_mu); the regularisation the first Gauss-Newton solve starts with */
    double  min_mu;              /* R: 1e-8 */
    double  max_mu;              /* R: 1.0 */
    double  mu_increase_factor;  /* R: 10 */
    double  increase_threshold;  /* R: 0.75 */
    double  decrease_threshold;  /* R: 0.25 */
    double  min_diagonal;        /* R: 1e-6 */
    double  max_diagonal;        /* R: 1e32 */
} lvi_win_params;

/* one IMUFactor: the state of its IntegrationBase.  Matrices are row-major 15 x 15 in the order O_P 0, O_R 3, O_V 6, O_BA 9,
 * O_BG 12 (parameters.h) */
typedef struct lvi_win_imu {
    int32_t pose_i, speed_bias_i, pose_j, speed_bias_j;   /* block ids: sizes 7, 9, 7, 9 */
    double  sum_dt;
    double  delta_p[3];
    double  delta_q[4];          /* x y z w */
    double  delta_v[3];
    double  linearized_ba[3], linearized_bg[3];
    double  jacobian[225];
    double  covariance[225];
} lvi_win_imu;

typedef struct lvi_win_info {
    int32_t iterations;          /* trust-region iterations run (the log holds iterations + 1 entries) */
    int32_t successful_steps;
    int32_t termination;         /* LVI_WIN_TERM_* */
    int32_t flags;               /* bit 0: a non-finite value; bit 1: an IMU covariance that is not positive definite */
    int32_t dim;                 /* D: columns of the reduced system */
    int32_t eliminated;
    double  initial_cost, final_cost;
    double  radius, mu;          /* as the loop left them */
    double  time_s;
} lvi_win_info;

typedef struct lvi_win_iteration {
    int32_t iteration;
    int32_t step_kind;           /* LVI_WIN_STEP_* */
    int32_t accepted;
    int32_t mu_retries;          /* factorisations that met a non-positive pivot in this iteration */
    double  cost;                /* of the state after the iteration */
    double  cost_change, model_cost_change, rho;
    double  gradient_max_norm;   /* of the state after the iteration */
    double  step_norm;           /* |delta| in the tangent space */
    double  radius, mu;          /* the step was computed with */
    double  gauss_newton_norm, cauchy_norm;   /* |D y_gn| and alpha |D^-1 g|: what the radius is compared with */
} lvi_win_iteration;

int32_t lvi_win_abi_version(void);
/* loss CAUCHY(1), sqrt_info 460 / 1.5, tr_over_row 0, half_row 240, G 0 0 9.8, max_iterations 8, max_time_s 0 and the R values above */
void lvi_win_params_default(lvi_win_params *p);

/* Every capacity is 1.. its LVI_WIN_MAX_* (max_eliminated, max_imu and max_prior_rows may be 0).  With P1 = max_dim + 1 device
 * memory grows as 8 P1^2 (ceil(max_projections / LVI_WIN_SHARE) + ceil((15 max_imu + max_prior_rows) / 256) + 3), 8 P1
 * (15 max_imu + max_prior_rows + max_eliminated), 8 max_prior_rows^2, 3.8 KB per IMU factor and 500 bytes per projection. */
int32_t lvi_win_create(int32_t device, const lvi_win_caps *caps, lvi_win **out);
void lvi_win_destroy(lvi_win *w);
int32_t lvi_win_set_params(lvi_win *w, const lvi_win_params *p);

/* ---- describing a problem.  Arguments are checked before anything is touched: an error leaves the description as it was. */
int32_t lvi_win_begin(lvi_win *w);                        /* forget the description (the prior included); the parameters stay */
/* AddParameterBlock (:703-717, :775-787).  size 1..LVI_WIN_MAX_BLOCK_SIZE; size 7 is a pose [p, q = x y z w] of local size 6
 * whose update is PoseLocalParameterization::Plus (pose_local_parameterization.cpp:3-19): p + dp, (q * deltaQ(dtheta))
 * .normalized().  The columns of the reduced system follow the order of declaration.  Declaring an id again with the same
 * size and flags replaces its values; otherwise LVI_ERR_INVALID_ARG. */
int32_t lvi_win_set_block(lvi_win *w, int32_t id, int32_t size, const double *values, int32_t flags);
/* :747-789: the five ids of a record must be declared, of sizes 7, 7, 7, 1, 1 (td == -1: ProjectionFactor) and distinct;
 * an LVI_WIN_ELIMINATED block may appear in the feature slot only */
int32_t lvi_win_add_projection(lvi_win *w, int32_t count, const lvi_marg_projection *records);
/* :735-744 (the sum_dt > 10 skip is the caller's).  sqrt_info = LLT(covariance^-1).matrixL()' (imu_factor.h:63) is computed
 * on the device once per solve; the covariance must be symmetric positive definite */
int32_t lvi_win_add_imu(lvi_win *w, int32_t count, const lvi_win_imu *records);
/* :719-726: the prior of a marginaliser on the same device, read where it lies: its linearized_jacobians,
 * linearized_residuals, keep_block_data and layout under the present (remapped) ids.  The handle must outlive the solve and
 * must not marginalise between this call and lvi_win_solve.  Every kept block must be declared here with its size and must
 * not be LVI_WIN_ELIMINATED: LVI_ERR_INVALID_ARG before anything is touched.  LVI_ERR_STATE when it has no result. */
int32_t lvi_win_set_prior_from_marg(lvi_win *w, lvi_marg *m);
/* the same from host arrays, as lvi_marg_get_prior and lvi_marg_get_layout return them: J row-major [n][n], r [n]; ids, sizes,
 * idx [count] with idx counted as keep_block_idx is (the smallest idx is the prior's column 0) and values
 * [count][LVI_WIN_MAX_BLOCK_SIZE]; the blocks' columns tile 0..n without overlap */
int32_t lvi_win_set_prior(lvi_win *w, int32_t n, const double *J, const double *r, int32_t count, const int32_t *ids, const int32_t *sizes,
                          const int32_t *idx, const double *values);

/* ceres::Solve (:806).  Returns LVI_OK, LVI_WIN_NOT_FINITE, LVI_WIN_BAD_COVARIANCE or an error (LVI_ERR_STATE without factors, LVI_ERR_CAPACITY when
 * the reduced system exceeds max_dim).  On LVI_OK the blocks hold the solution; the description stays, so a second
 * lvi_win_solve continues from it.  info_out may be NULL. */
int32_t lvi_win_solve(lvi_win *w, lvi_win_info *info_out);
int32_t lvi_win_get_block(lvi_win *w, int32_t id, double *values);
/* the iterations of the last solve, entry 0 being the state it started from; cap: the room of log (may be NULL) */
int32_t lvi_win_get_log(lvi_win *w, int32_t cap, int32_t *count, lvi_win_iteration *log);
/* for tests: the system at the blocks' current values, before scaling and regularisation.  *dim = D, *eliminated = E,
 * *dense_rows = the rows of the IMU factors and the prior together; H row-major [D][D] and g [D] are the camera-side J'J and
 * J'r before the elimination, hdiag [E] and gf [E] the eliminated diagonal and gradient, W row-major [E][D] the coupling;
 * proj_rows [count][2][21]: the loss-corrected Jacobian rows (20 columns as csrc/lvi_marg_math.hpp orders them) and
 * residual of every projection factor; dense [dense_rows][D + 1]: the rows of the IMU factors, then of the prior, over the
 * reduced columns with the residual last.  Every array may be NULL; cap_dim, cap_elim, cap_proj, cap_dense: their room,
 * LVI_ERR_CAPACITY when one that is given is too short. */
int32_t lvi_win_debug_system(lvi_win *w, int32_t cap_dim, int32_t cap_elim, int32_t cap_proj, int32_t cap_dense, int32_t *dim, int32_t *eliminated,
                             int32_t *dense_rows, double *H, double *g, double *hdiag, double *gf, double *W, double *proj_rows, double *dense, double *cost);

#ifdef __cplusplus
}
#endif
#endif /* LVI_WIN_H */
