"""float64 numpy reference of the pose graph WITH GPS factors and of its marginal covariance (include/lvi_pgo_gps.h, DESIGN
§19): pgo_ref's graph plus the gtsam::GPSFactor of mapOptimization.cpp:1497-1499 and isam->marginalCovariance of :1591.

GPSFactor (recalled, like the rest of pgo_ref): error = X.translation() - z, Jacobian with respect to the right
perturbation (rotation, translation) = [0 | R], whitened by 1 / sqrt(variance) per axis.  It is the first factor that is
not blind to a common left transform of all poses, so a graph that holds one has no gauge direction left to anchor: the
step is the full system's, with both linear solvers of pgo_ref, and it converges because the GPS information (about 1)
replaces the 1e-8 of the translation prior as the weakest entry.  A graph without a GPS factor steps exactly as pgo_ref
does.

The marginal covariance of key k is the (k, k) block of (J'J)^-1, J the whitened Jacobian of ALL factors at the current
poses.  Two independent routes each:
  with GPS      "qr"    R of a QR factorisation of J (never forms J'J): block = Y'Y, R'Y = E_k
                "chol"  Cholesky of J'J and two triangular solves
  without GPS   "qr"    the same
                "split" the gauge split: Sigma_k = A (Bp' W Bp)^-1 A' + Sigma_rel,k, A = Ad(X_k^-1 X_0), Bp the prior's
                        Jacobian, W its information, Sigma_rel,k the block of the anchored system (key 0 removed, the
                        prior's rows removed; zero for key 0).  The step of key 0 is the prior's alone (pgo_ref's
                        docstring), every other key's is Ad(X_k^-1 X_0) delta_0 plus a part that depends on the between
                        factors only, and the two parts are independent.
inv(J'J) without GPS is NOT a route: cond(J'J) is 2.6e16 (n37) to 1.1e18 (n300) and its block is off by 2e-3 to 4e-3
relative, which test_pgo_gps_ref.py measures."""
import numpy as np

import pgo_ref as R

F32, F64 = np.float32, np.float64
GPS_MAX_ITERS = 30


def gps_error(X, z):
    """-> (r [3], J [3, 6])"""
    J = np.zeros((3, 6))
    J[:, 3:] = X[:3, :3]
    return X[:3, 3] - z, J


class GpsGraph(R.Graph):
    """pgo_ref.Graph plus the calls of include/lvi_pgo_gps.h"""

    def __init__(self, full_logmap=1, conv_eps=R.CONV_EPS, max_iters=R.MAX_ITERS):
        super().__init__(full_logmap, conv_eps, max_iters)
        self.gps = []

    def copy(self):
        g = GpsGraph(self.full, self.eps, self.max_iters)
        g.X, g.Zc, g.loops, g.gps = [x.copy() for x in self.X], list(self.Zc), list(self.loops), list(self.gps)
        return g

    def add_gps(self, key, xyz, variance):
        z, v = np.asarray(xyz, F32).astype(F64).reshape(3), np.asarray(variance, F32).astype(F64).reshape(3)
        if not 0 <= key < len(self.X) or not np.isfinite(z).all() or not np.isfinite(v).all() or not (v > 0).all():
            raise ValueError("bad GPS factor")
        self.gps.append((int(key), z, v))

    def gps_count(self):
        return len(self.gps)

    def gps_rows(self):
        """(key, whitened r [3], whitened J [3, 6]) per factor"""
        out = []
        for key, z, v in self.gps:
            r, J = gps_error(self.X[key], z)
            s = 1. / np.sqrt(v)
            out.append((key, s * r, s[:, None] * J))
        return out

    def chi2(self):
        # prior, chain, loops, then GPS
        return float(super().chi2() + sum(np.dot(r, r) for _, r, _ in self.gps_rows()))

    def linear_system(self, sparse):
        J, r = super().linear_system(sparse)
        rows = self.gps_rows()
        if not rows:
            return J, r
        n = len(self.X)
        Jg = np.zeros((3 * len(rows), 6 * n))
        rg = np.zeros(3 * len(rows))
        for e, (key, re, Je) in enumerate(rows):
            Jg[3 * e:3 * e + 3, 6 * key:6 * key + 6] = Je
            rg[3 * e:3 * e + 3] = re
        if sparse:
            import scipy.sparse as sp
            return sp.vstack([J, sp.csc_matrix(Jg)], format="csc"), np.r_[r, rg]
        return np.vstack([J, Jg]), np.r_[r, rg]

    def step(self, solver, gauge="anchored"):
        """with a GPS factor: the full system, whatever `gauge` says (there is no gauge); without: pgo_ref's step"""
        return super().step(solver, "full" if self.gps else gauge)

    # ---- the marginal covariance ----------------------------------------------------------------------
    def _dense_system(self):
        J, _ = self.linear_system(False)
        return J

    def marginal_covariance(self, key, route):
        n = len(self.X)
        if not 0 <= key < n:
            raise ValueError("bad key")
        J = self._dense_system()
        if route == "split":
            if self.gps:
                raise ValueError("the gauge split holds only without GPS factors")
            _, Bp = R.prior_error(self.X[0], self.Zc[0], self.full)
            Bi = np.linalg.inv(Bp)                                         # cond(Bp) is O(1): Jr^-1 of a small error
            S0 = Bi @ np.diag(R.PRIOR_VAR) @ Bi.T
            A = R.adjoint(R.pose_inv(self.X[key]) @ self.X[0])
            C = A @ S0 @ A.T
            if key > 0:
                C = C + _block_by_qr(J[6:, 6:], key - 1)
            return C
        if route == "qr":
            return _block_by_qr(J, key)
        if route == "chol":
            L = np.linalg.cholesky(J.T @ J)
            E = np.zeros((6 * n, 6))
            E[6 * key:6 * key + 6] = np.eye(6)
            import scipy.linalg as sl
            Y = sl.solve_triangular(L, E, lower=True)
            return Y.T @ Y
        if route == "inv":                                                # the route that is NOT one without GPS (measured in the CPU tier)
            return np.linalg.inv(J.T @ J)[6 * key:6 * key + 6, 6 * key:6 * key + 6]
        raise ValueError(route)


def _block_by_qr(J, key):
    """the (key, key) block of (J'J)^-1 from the R of J = Q R: R'Y = E_key, block = Y'Y"""
    import scipy.linalg as sl
    Rm = np.linalg.qr(J, mode="r")
    E = np.zeros((J.shape[1], 6))
    E[6 * key:6 * key + 6] = np.eye(6)
    Y = sl.solve_triangular(Rm, E, trans="T", lower=False)
    return Y.T @ Y


def abs_gaps(Xa, Xb):
    """(rotation angle, translation) of the largest Xa_i^-1 Xb_i over ALL keys: GPS fixes the gauge, key 0 is not special"""
    ra = ta = 0.0
    for a, b in zip(Xa, Xb):
        D = R.pose_inv(a) @ b
        ra, ta = max(ra, R.rot_angle(D[:3, :3])), max(ta, float(np.linalg.norm(D[:3, 3])))
    return ra, ta


def cov_gap(Ca, Cb):
    """largest |Ca - Cb| relative to max|Ca|"""
    return float(np.abs(Ca - Cb).max() / np.abs(Ca).max())


# ---- scenes ---------------------------------------------------------------------------------------------
GPS_SIGMA, GPS_VAR, GPS_SEED = 0.3, (1.0, 2.0, 1.0), 11
N37_LOOPS = R.GPU_SCENES["n37"][1]
# name -> (keys or the name of a pgo_ref GPU scene, loops (from, to), keys that carry a GPS factor)
GPS_SCENES = {
    "g5": (5, [], [4]),                                                  # key 0 live, only the single-workgroup tail of the reduction
    "g12": (12, [(11, 0)], [11]),
    "g20_mid": (20, [(19, 2)], [10]),                                    # the last key's (3,3) stays above 25 although a fix exists
    "g37_key0": (37, N37_LOOPS, [0]),                                    # prior and GPS on the same key
    "g37_twice": (37, [(36, 0)], [36, 36]),                              # two factors on one key
    "g64": (64, [(63, 1), (40, 7)], [20, 63]),                           # 13 undamped steps in both charts: more than the default max_iters
    "g300": ("n300", None, [100, 200, 299] + list(range(0, 300, 7))),    # the multi-launch reduction levels
}


def gps_scene(name):
    """pgo_ref's scene dict plus gps = [(key, xyz f32 [3], variance f32 [3])]: ground-truth position + N(0, GPS_SIGMA)"""
    n, loops, keys = GPS_SCENES[name]
    sc = R.gpu_scene(n) if isinstance(n, str) else R.scene(n, loops, GPS_SEED)
    rs = np.random.RandomState(GPS_SEED)                                  # a fresh stream per scene
    sc = dict(sc)
    sc["gps"] = [(k, (sc["gt"][k][:3, 3] + rs.normal(0, GPS_SIGMA, 3)).astype(F32), np.array(GPS_VAR, F32)) for k in keys]
    return sc


def build(sc, g):
    """feed a scene to a graph-like object (add_pose / add_loop / add_gps)"""
    R.build(sc, g)
    for key, xyz, var in sc.get("gps", []):
        g.add_gps(key, xyz, var)
    return g


def solve_both(g):
    """as pgo_ref.solve_both: ((poses, info) of lstsq, (poses, info) of chol); g itself takes the lstsq answer"""
    return R.solve_both(g)
