/* lvi_marg.h — the marginalisation of vins_estimator's sliding window on the GPU: MarginalizationInfo.
 *
 * Replaces what Estimator::optimization does after the window solve (estimator.cpp:813-976): addResidualBlockInfo,
 * preMarginalize and marginalize of marginalization_factor.cpp (:89-129, :174-296), getParameterBlocks (:298-318) and the
 * evaluation of the previous prior as a MarginalizationFactor (:332-380).  The projection factors (projection_factor.cpp:21-121,
 * projection_td_factor.cpp:34-141) and the loss correction of ResidualBlockInfo::Evaluate (:37-68) are evaluated on the
 * device; IMUFactor is handed in evaluated (lvi_marg_add_dense).  The contract is DESIGN §21.
 * Exported by liblvi_hip.so only (the CPU oracle does not implement it); a separate ABI from lvi_hotpath.h, whose version
 * it does not change.  All arithmetic is double.
 *
 * Parameter blocks are named by caller-chosen int32 ids where the reference uses addresses.  The reference orders the
 * blocks by iterating an unordered_map keyed by address, which is unspecified; here the order is: dropped blocks in order
 * of first appearance in a drop set, then kept blocks in order of first appearance in a factor; a declared block that no
 * factor names is not part of the system.  The result therefore differs from any reference run by a column permutation
 * only (and the rows of linearized_jacobians follow ascending eigenvalues, as Eigen sorts them); keep_block_idx travels
 * with it (lvi_marg_get_layout).
 *
 * The prior stays on the device: the next marginalisation consumes it through lvi_marg_add_last_prior, and only the
 * window's parameter values and the new observations go up.
 */
#ifndef LVI_MARG_H
#define LVI_MARG_H

#include "lvi_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_MARG_ABI_VERSION         1
#define LVI_MARG_MAX_BLOCKS          2048   /* upper bound of caps.max_blocks */
#define LVI_MARG_MAX_PROJECTIONS     8192   /* ... of caps.max_projections */
#define LVI_MARG_MAX_DENSE_FACTORS   16     /* ... of caps.max_dense_factors */
#define LVI_MARG_MAX_DENSE_ROWS      256    /* ... of caps.max_dense_rows (all dense factors together) */
#define LVI_MARG_MAX_DROP_DIM        512    /* ... of caps.max_drop_dim, the reference's m */
#define LVI_MARG_MAX_KEEP_DIM        256    /* ... of caps.max_keep_dim, the reference's n */
#define LVI_MARG_MAX_BLOCK_SIZE      16     /* global size of a parameter block */
#define LVI_MARG_MAX_SWEEPS          64     /* upper bound of params.max_sweeps */
#define LVI_MARG_SHARE               128    /* projection factors one workgroup accumulates before its partial is written */

/* loss functions of params.loss_type */
#define LVI_MARG_LOSS_NONE           0
#define LVI_MARG_LOSS_CAUCHY         1      /* ceres::CauchyLoss(loss_a), the reference's (estimator.cpp:701) */
#define LVI_MARG_LOSS_HUBER          2      /* ceres::HuberLoss(loss_a), its commented alternative */

/* soft status of lvi_marg_marginalize (> 0) */
#define LVI_MARG_EIG_NOT_CONVERGED   1      /* an eigen-solver took max_sweeps sweeps; the result is installed as it stands */
#define LVI_MARG_NOT_FINITE          2      /* the system or the result has a non-finite entry (inv_dep == 0, dep_j == 0); the
                                               previous prior stays in place */

typedef struct lvi_marg lvi_marg;

typedef struct lvi_marg_caps {
    int32_t max_blocks;          /* parameter blocks declared between two lvi_marg_begin */
    int32_t max_projections;     /* projection factors */
    int32_t max_dense_factors;   /* factors the caller evaluates */
    int32_t max_dense_rows;      /* their rows, all together */
    int32_t max_drop_dim;        /* m: the local size of everything dropped */
    int32_t max_keep_dim;        /* n: the local size of everything kept */
} lvi_marg_caps;

typedef struct lvi_marg_params {
    int32_t loss_type;           /* LVI_MARG_LOSS_*: the loss of the projection factors */
    int32_t max_sweeps;          /* sweep bound of the eigen-solver (1..LVI_MARG_MAX_SWEEPS) */
    double  loss_a;              /* the loss's scale a (> 0) */
    double  sqrt_info;           /* ProjectionFactor::sqrt_info = FOCAL_LENGTH / 1.5 * I (estimator.cpp:17-18) */
    double  tr_over_row;         /* TR / ROW, the rolling-shutter read-out time per line over the image height */
    double  half_row;            /* ROW / 2: row = uv.y - ROW / 2 (projection_td_factor.cpp:18-19) */
    double  eps;                 /* the eigenvalue threshold of both pseudo-inverses (marginalization_factor.h: 1e-8) */
} lvi_marg_params;

/* one ProjectionTdFactor (td >= 0) or ProjectionFactor (td == -1, velocities, td_i, td_j and rows unused) */
typedef struct lvi_marg_projection {
    int32_t pose_i, pose_j, ex, feature, td;   /* block ids: sizes 7, 7, 7, 1, 1 */
    int32_t reserved;
    double  pts_i[3], pts_j[3];
    double  velocity_i[2], velocity_j[2];
    double  td_i, td_j;
    double  row_i, row_j;                      /* uv.y of the two observations */
} lvi_marg_projection;

typedef struct lvi_marg_info {
    int32_t m, n, rank;          /* dropped and kept local sizes; eigenvalues of the Schur complement above eps */
    int32_t rank_mm;             /* eigenvalues of Amm above eps */
    int32_t sweeps_mm, sweeps_rr;/* sweeps the two eigen-solves took */
    int32_t flags;               /* bit 0: an eigen-solve hit max_sweeps; bit 1: a non-finite entry */
    int32_t kept_blocks;
    double  cost;                /* sum of squared (loss-corrected) residuals at the linearisation point */
    double  off_mm, off_rr;      /* largest |off-diagonal| the last sweep of each eigen-solve met */
} lvi_marg_info;

int32_t lvi_marg_abi_version(void);
/* loss_type CAUCHY, loss_a 1, max_sweeps 30, sqrt_info 460 / 1.5, tr_over_row 0, half_row 240, eps 1e-8 */
void lvi_marg_params_default(lvi_marg_params *p);

/* Every capacity is 1.. its LVI_MARG_MAX_* (max_dense_factors and max_dense_rows may be 0).  With P = max_drop_dim +
 * max_keep_dim + 1, device memory grows as 8 P^2 (ceil(max_projections / LVI_MARG_SHARE) + ceil((max_dense_rows +
 * max_keep_dim) / 256) + 1) bytes for the partial sums, plus 8 P (max_dense_rows + max_keep_dim) for the dense rows, 24
 * max_drop_dim^2, 16 max_drop_dim max_keep_dim and 40 max_keep_dim^2 for the eigen-solves and the two priors, and 496 bytes per projection. */
int32_t lvi_marg_create(int32_t device, const lvi_marg_caps *caps, lvi_marg **out);
void lvi_marg_destroy(lvi_marg *m);
int32_t lvi_marg_clear(lvi_marg *m);                       /* no prior, nothing described; the parameters stay */
int32_t lvi_marg_set_params(lvi_marg *m, const lvi_marg_params *p);

/* ---- describing a marginalisation.  Arguments are checked before anything is touched: an error leaves the handle, its
 * description so far and its prior as they were. */
int32_t lvi_marg_begin(lvi_marg *m);                       /* forget the description; the prior stays */
/* a parameter block and its current values.  size 1..LVI_MARG_MAX_BLOCK_SIZE; the local size is size, except 7 -> 6 (the
 * reference's localSize, :131-134): [p (3), q = x y z w (4)].  Declaring an id again with the same size replaces its values;
 * with another size: LVI_ERR_INVALID_ARG. */
int32_t lvi_marg_set_block(lvi_marg *m, int32_t id, int32_t size, const double *values);
/* estimator.cpp:861-888: count factors, evaluated on the device, loss params.loss_type, drop set {0, 3} (:877, :885):
 * pose_i and the feature are dropped.  The five ids of a record must be declared, of sizes 7, 7, 7, 1, 1, and distinct. */
int32_t lvi_marg_add_projection(lvi_marg *m, int32_t count, const lvi_marg_projection *records);
/* a factor the caller evaluated, without loss (IMUFactor, :837-844): residual [n_rows]; jacobians: for block 0, 1, ... in
 * turn a row-major [n_rows][size of the block] matrix as ceres fills it (the 7th column of a size-7 block is ignored);
 * drop_mask [n_blocks]: non-zero drops the block. */
int32_t lvi_marg_add_dense(lvi_marg *m, int32_t n_rows, int32_t n_blocks, const int32_t *ids, const double *residual, const double *jacobians,
                           const int32_t *drop_mask);
/* the previous result of this handle as a MarginalizationFactor (:818-834, :924-940), evaluated on the device at the
 * declared values of its kept blocks (:332-380; dx of a size-7 block is 2 (q0^-1 q).vec(), negated when (q0^-1 q).w < 0);
 * nothing is downloaded or uploaded for it.  Every kept block of the prior must be declared under its (remapped) id with
 * its size; drop_ids [n_drop] must be among them.  LVI_ERR_STATE without a previous result or when given twice. */
int32_t lvi_marg_add_last_prior(lvi_marg *m, int32_t n_drop, const int32_t *drop_ids);

/* preMarginalize + marginalize (:110-129, :174-296).  Everything is enqueued at once and waited for once: factor
 * evaluation; A = sum J'J and b = sum J'r in a fixed order (no floating-point atomics: two runs give the same bits); Amm =
 * (Amm + Amm') / 2; a symmetric eigendecomposition of the whole Amm and its pseudo-inverse above eps (:266-271); the Schur
 * complement (:274-280); its eigendecomposition; linearized_jacobians = sqrt(S) V' and linearized_residuals = sqrt(S_inv)
 * V' b (:282-290).  Returns LVI_OK, a soft status, or an error (LVI_ERR_STATE when nothing is dropped or nothing is kept,
 * LVI_ERR_CAPACITY when m or n exceed the capacities).  On LVI_OK and LVI_MARG_EIG_NOT_CONVERGED the result becomes the
 * handle's prior and the description is consumed; otherwise the previous prior stays.  info_out may be NULL. */
int32_t lvi_marg_marginalize(lvi_marg *m, lvi_marg_info *info_out);

/* ---- after the call */
/* getParameterBlocks (:298-318): the kept blocks in their order: ids, sizes (global), idx (the reference's keep_block_idx:
 * the block's first column counted from the start of the dropped part, so idx - m is its column in the prior) and
 * values [count][LVI_MARG_MAX_BLOCK_SIZE], the reference's keep_block_data.  cap: the room of the arrays (each may be
 * NULL); *count = the number of kept blocks.  LVI_ERR_STATE without a prior. */
int32_t lvi_marg_get_layout(lvi_marg *m, lvi_marg_info *info, int32_t cap, int32_t *count, int32_t *ids, int32_t *sizes, int32_t *idx, double *values);
/* linearized_jacobians (row-major [n][n]) and linearized_residuals [n], for a caller whose Ceres still runs the window
 * optimisation.  Either may be NULL. */
int32_t lvi_marg_get_prior(lvi_marg *m, double *jacobians, double *residuals);
/* addr_shift of :896-913 and :946-973: the kept block with id old_ids[k] is known as new_ids[k] from now on; kept blocks
 * not listed keep their ids.  Two kept blocks under one id: LVI_ERR_INVALID_ARG.  Between lvi_marg_add_last_prior and
 * lvi_marg_marginalize the result is part of the description under its present ids: LVI_ERR_STATE. */
int32_t lvi_marg_remap(lvi_marg *m, const int32_t *old_ids, const int32_t *new_ids, int32_t count);
/* the full system of the last lvi_marg_marginalize that reached the device (a LVI_MARG_NOT_FINITE one included) before the
 * Schur step, for tests: *pos = m + n of that call; A row-major [pos][pos], b [pos], both may be NULL; cap: the rows the
 * arrays have room for, LVI_ERR_CAPACITY when that is less than pos and one of them is given */
int32_t lvi_marg_debug_system(lvi_marg *m, int32_t cap, int32_t *pos, double *A, double *b);

#ifdef __cplusplus
}
#endif
#endif /* LVI_MARG_H */
