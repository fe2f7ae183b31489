/* lvi_pgo_gps.h — GPS factors of mapOptimization's factor graph and the covariance that gates them, on the GPU.
 *
 * Replaces the graph side of addGPSFactor (mapOptimization.cpp:1430-1507: the gtsam::GPSFactor of :1497-1499) and
 * poseCovariance = isam->marginalCovariance(latest key) (:1591).  The decisions of addGPSFactor around the factor (the
 * queue, the time window, the thresholds, the 5 m spacing, max(noise, 1.0f)) are host work: host/lvi_gps_gate.hpp.
 * An extension of include/lvi_pgo.h that operates on its handle: lvi_pgo.h, its 11 functions, its two records and
 * LVI_PGO_ABI_VERSION do not change.  Exported by liblvi_hip.so only.  The contract is DESIGN §19.
 *
 * GPSFactor (GTSAM, restated from memory like the rest of DESIGN §18): error = X.translation() - measured, its Jacobian
 * with respect to the right perturbation (rotation, translation) is [0 | R], whitened by 1 / sqrt(variance) per axis.
 * It is the one factor that is not invariant under a common left transform of all poses, so a graph that holds one is
 * solved as the full system: key 0 is a live key of the chain, not "the prior's alone" (DESIGN §19).  A graph without one
 * takes exactly the path of lvi_pgo.h.
 */
#ifndef LVI_PGO_GPS_H
#define LVI_PGO_GPS_H

#include "lvi_pgo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_PGO_GPS_ABI_VERSION 1

int32_t lvi_pgo_gps_abi_version(void);

/* gtSAMgraph.add(GPSFactor(key, Point3(x, y, z), Variances(variance))) (:1497-1499).  key: any key added so far; several
 * factors may sit on one key.  xyz and variance are kept as the doubles of the floats handed in; the variances are not
 * clamped here (max(noise, 1.0f) of :1495 is the caller's).  A key outside the keys added so far, a variance <= 0 or not
 * finite, a coordinate that is not finite: LVI_ERR_INVALID_ARG; more than max_poses factors in total: LVI_ERR_CAPACITY.
 * The arguments are checked before anything is touched and an error leaves all state as it was.  lvi_pgo_clear removes
 * the GPS factors too.  With at least one GPS factor lvi_pgo_solve (:1546-1566) minimises the cost that includes them,
 * and chi2_before / chi2_after sum prior, chain, loops, GPS in that order. */
int32_t lvi_pgo_gps_add(lvi_pgo *g, int32_t key, const float xyz[3], const float variance[3]);

/* the number of GPS factors the graph holds (what :1430-1507 has added since the last lvi_pgo_clear) */
int32_t lvi_pgo_gps_count(lvi_pgo *g, int32_t *n_gps);

/* isam->marginalCovariance(key) (:1591): the (key, key) 6x6 block of the inverse of the whitened normal matrix of ALL
 * factors, linearised at the poses the handle holds now (iSAM2 linearises at its own linearisation point: DESIGN §19).
 * cov: row-major, tangent order rotation then translation, so (3,3) and (4,4) — what :1443 reads — are x and y in the
 * key's body frame.  Takes no step and changes no pose; one pass of the solver's kernels with six unit right-hand sides,
 * no linear algebra on the host, one wait.  Without GPS factors the prior's part is applied in closed form
 * (Ad (Bp' W Bp)^-1 Ad' + the block of the anchored system), never by inverting a system that holds 1e-8 beside 1e6.
 * LVI_ERR_STATE without poses, LVI_ERR_INVALID_ARG for a key outside the keys added so far. */
int32_t lvi_pgo_gps_marginal_covariance(lvi_pgo *g, int32_t key, double cov[36]);

#ifdef __cplusplus
}
#endif
#endif /* LVI_PGO_GPS_H */
