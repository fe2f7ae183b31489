"""Reference of the feature table (include/lvi_fman.h): a restatement of vins_estimator's FeatureManager
(feature_manager.{h,cpp}) and of the two factor loops of Estimator::optimization (estimator.cpp:745-789, :849-889) as a
plain-Python class over a list, in float64.  Every sum is written out term by term with Python floats, left to right, so
that nothing is fused or reordered: apart from the triangulated depth the device must give these bits.  The triangulation
is given twice: by numpy.linalg.svd, and in mpmath at 80 digits (the smallest eigenvector of A'A, which at 80 digits keeps
40 and more).  Seeded scene generators are at the end.  Nothing here reads the library."""
import math

import mpmath as mp
import numpy as np

WINDOW, MAX_OBS = 10, 11
INIT_DEPTH, MIN_PARALLAX = 5.0, 10.0 / 460.0
MODE_WINDOW, MODE_MARG_OLD = 0, 1
ID_POSE, ID_EX, ID_TD, ID_FEATURE = 0, 32, 33, 64      # VinsMarginalizer::ID_*
MP_DIGITS = 80
FOCAL = 460.0


# ---- 3 x 3 arithmetic, every entry (t0 + t1) + t2 ----------------------------------------------------------------
def mul33(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def mul33t(A, B):
    """A' B"""
    return [[A[0][i] * B[0][j] + A[1][i] * B[1][j] + A[2][i] * B[2][j] for j in range(3)] for i in range(3)]


def mul3v(A, x):
    return [A[i][0] * x[0] + A[i][1] * x[1] + A[i][2] * x[2] for i in range(3)]


def mul3tv(A, x):
    return [A[0][i] * x[0] + A[1][i] * x[1] + A[2][i] * x[2] for i in range(3)]


def _mat(R, num=float):
    return [[num(R[i][j]) for j in range(3)] for i in range(3)]


def std_max(a, b):
    return b if a < b else a


def std_min(a, b):
    return b if b < a else a


def eligible(n_obs, start_frame):
    """getFeatureCount's rule (feature_manager.cpp:36)"""
    return n_obs >= 2 and start_frame < WINDOW - 2


def compensated_parallax2(p_i, p_j):
    """feature_manager.cpp:381-414 as written"""
    ans = 0.0
    u_j, v_j = p_j[0], p_j[1]
    dep_i = p_i[2]
    u_i, v_i = p_i[0] / dep_i, p_i[1] / dep_i
    du, dv = u_i - u_j, v_i - v_j
    dep_i_comp = p_i[2]
    u_i_comp, v_i_comp = p_i[0] / dep_i_comp, p_i[1] / dep_i_comp
    du_comp, dv_comp = u_i_comp - u_j, v_i_comp - v_j
    return std_max(ans, math.sqrt(std_min(du * du + dv * dv, du_comp * du_comp + dv_comp * dv_comp)))


def shifted_depth(uv_i, depth, marg_R, marg_P, new_R, new_P):
    """dep_j of removeBackShiftDepth (:314-317)"""
    pts_i = [uv_i[0] * depth, uv_i[1] * depth, uv_i[2] * depth]
    w = mul3v(marg_R, pts_i)
    d = [(w[k] + marg_P[k]) - new_P[k] for k in range(3)]
    return new_R[0][2] * d[0] + new_R[1][2] * d[1] + new_R[2][2] * d[2]


# ---- triangulation ------------------------------------------------------------------------------------------------
def triangulation_rows(Ps, Rs, tic, ric, start, points, num=float, sqrt=math.sqrt):
    """the 2k x 4 matrix of triangulate (:223-252) in the arithmetic of `num`, from float64 inputs"""
    Ps = [[num(v) for v in p] for p in Ps]
    Rs = [_mat(R, num) for R in Rs]
    tic, ric = [num(v) for v in tic], _mat(ric, num)
    v = mul3v(Rs[start], tic)
    t0 = [Ps[start][c] + v[c] for c in range(3)]
    R0 = mul33(Rs[start], ric)
    rows = []
    for o, p in enumerate(points):
        j = start + o
        v = mul3v(Rs[j], tic)
        t1 = [Ps[j][c] + v[c] for c in range(3)]
        R1 = mul33(Rs[j], ric)
        t = mul3tv(R0, [t1[c] - t0[c] for c in range(3)])
        R = mul33t(R0, R1)
        Rt_t = mul3tv(R, t)
        P = [[R[0][r], R[1][r], R[2][r], -Rt_t[r]] for r in range(3)]
        p = [num(c) for c in p[:3]]
        z = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
        f = p
        if z > 0:
            n = sqrt(z)
            f = [p[0] / n, p[1] / n, p[2] / n]
        rows.append([f[0] * P[2][c] - f[2] * P[0][c] for c in range(4)])
        rows.append([f[1] * P[2][c] - f[2] * P[1][c] for c in range(4)])
    return rows


def depth_numpy(Ps, Rs, tic, ric, start, points):
    """-> (svd_V[2] / svd_V[3], singular values) by numpy.linalg.svd in float64"""
    A = np.array(triangulation_rows(Ps, Rs, tic, ric, start, points), np.float64)
    _, s, vt = np.linalg.svd(A)
    v = vt[-1]
    with np.errstate(all="ignore"):
        return float(np.float64(v[2]) / np.float64(v[3])), s


def depth_mp(Ps, Rs, tic, ric, start, points):
    """the same in mpmath at MP_DIGITS digits -> mpf"""
    with mp.workdps(MP_DIGITS):
        A = mp.matrix(triangulation_rows(Ps, Rs, tic, ric, start, points, mp.mpf, mp.sqrt))
        E, Q = mp.eigsy(A.T * A)
        k = min(range(4), key=lambda c: E[c])
        return Q[2, k] / Q[3, k] if Q[3, k] != 0 else mp.nan              # a degenerate feature has no reference depth


def rel_dev(value, exact):
    """|value - exact| / |exact| of a float64 against an mpf"""
    with mp.workdps(MP_DIGITS):
        return float(abs(mp.mpf(value) - exact) / abs(exact))


# ---- the manager ----------------------------------------------------------------------------------------------------
class Feature:
    """FeaturePerId; an observation is [x, y, z, u, v, vx, vy, depth, cur_td]"""

    def __init__(self, feature_id, start_frame, measured_depth):
        self.feature_id, self.start_frame, self.obs, self.solve_flag = int(feature_id), int(start_frame), [], 0
        if measured_depth > 0:                               # feature_manager.h:60-74
            self.estimated_depth, self.lidar_depth_flag = measured_depth, True
        else:
            self.estimated_depth, self.lidar_depth_flag = -1.0, False

    def end_frame(self):
        return self.start_frame + len(self.obs) - 1


class FeatureManager:
    def __init__(self, init_depth=INIT_DEPTH, min_parallax=MIN_PARALLAX):
        self.feature, self.last_track_num = [], 0
        self.init_depth, self.min_parallax = float(init_depth), float(min_parallax)

    def clear_state(self):
        self.feature = []

    def get_feature_count(self):
        return sum(1 for f in self.feature if eligible(len(f.obs), f.start_frame))

    def add_frame(self, frame_count, ids, obs, td):
        """addFeatureCheckParallax (:45-106) -> dict(last_track_num, parallax_num, keyframe, added, parallax_sum)"""
        ids = [int(i) for i in ids]
        assert all(a < b for a, b in zip(ids, ids[1:])), "a std::map iterates in ascending key order"
        parallax_sum, parallax_num, added = 0.0, 0, 0
        self.last_track_num = 0
        for fid, o in zip(ids, obs):
            per_frame = [float(v) for v in o[:8]] + [float(td)]
            it = next((f for f in self.feature if f.feature_id == fid), None)
            if it is None:
                self.feature.append(Feature(fid, frame_count, per_frame[7]))
                self.feature[-1].obs.append(per_frame)
                added += 1
            else:
                it.obs.append(per_frame)
                self.last_track_num += 1
                if per_frame[7] > 0 and not it.lidar_depth_flag:
                    it.estimated_depth = per_frame[7]
                    it.lidar_depth_flag = True
                    it.obs[0][7] = per_frame[7]
        info = dict(last_track_num=self.last_track_num, parallax_num=0, keyframe=1, added=added, parallax_sum=0.0)
        if frame_count < 2 or self.last_track_num < 20:
            return info
        for f in self.feature:
            if f.start_frame <= frame_count - 2 and f.start_frame + len(f.obs) - 1 >= frame_count - 1:
                parallax_sum += compensated_parallax2(f.obs[frame_count - 2 - f.start_frame], f.obs[frame_count - 1 - f.start_frame])
                parallax_num += 1
        info.update(parallax_num=parallax_num, parallax_sum=parallax_sum)
        if parallax_num != 0:
            info["keyframe"] = 1 if parallax_sum / parallax_num >= self.min_parallax else 0
        return info

    def corresponding(self, l, r):
        """getCorresponding (:129-148); an index outside the observations (undefined there) yields no pair"""
        out = []
        for f in self.feature:
            if f.start_frame <= l and f.end_frame() >= r and l - f.start_frame < len(f.obs) and r >= f.start_frame:
                out.append([f.obs[l - f.start_frame][:3], f.obs[r - f.start_frame][:3]])
        return out

    def _eligible(self):
        return [f for f in self.feature if eligible(len(f.obs), f.start_frame)]

    def set_depth(self, x):
        fs = self._eligible()
        assert len(x) == len(fs)
        for f, v in zip(fs, x):
            with np.errstate(all="ignore"):
                f.estimated_depth = float(np.float64(1.0) / np.float64(v))
            f.solve_flag = 2 if f.estimated_depth < 0 else 1

    def clear_depth(self, x):
        fs = self._eligible()
        assert len(x) == len(fs)
        for f, v in zip(fs, x):
            with np.errstate(all="ignore"):
                f.estimated_depth = float(np.float64(1.0) / np.float64(v))
            f.lidar_depth_flag = False

    def remove_failures(self):
        self.feature = [f for f in self.feature if f.solve_flag != 2]

    def depth_vector(self):
        return [1.0 / f.estimated_depth if f.estimated_depth > 0 else 1.0 / self.init_depth for f in self._eligible()]

    def to_triangulate(self):
        """the features that pass the skip rule of :218-222, in list order"""
        return [f for f in self._eligible() if not f.estimated_depth > 0]

    def triangulate(self, Ps, Rs, tic, ric, depth_of=None):
        """triangulate (:213-268); depth_of(feature) -> svd_method, by default numpy's SVD"""
        done = []
        for f in self.to_triangulate():
            d = depth_of(f) if depth_of else depth_numpy(Ps, Rs, tic, ric, f.start_frame, f.obs)[0]
            f.estimated_depth = d
            if f.estimated_depth < 0.0:
                f.estimated_depth = self.init_depth
            done.append(f)
        return done

    def remove_back_shift_depth(self, marg_R, marg_P, new_R, new_P):
        """:285-339 -> the outcomes met, for the tests: 'lidar', 'dep_j', 'init', 'erased', 'shifted'"""
        marg_R, new_R = _mat(marg_R), _mat(new_R)
        marg_P, new_P = [float(v) for v in marg_P], [float(v) for v in new_P]
        kept, seen = [], []
        for f in self.feature:
            if f.start_frame != 0:
                f.start_frame -= 1
                kept.append(f)
                seen.append("shifted")
                continue
            uv_i = f.obs[0][:3]
            depth = -1.0
            if f.obs[0][7] > 0:
                depth = f.obs[0][7]
            elif f.estimated_depth > 0:
                depth = f.estimated_depth
            del f.obs[0]
            if len(f.obs) < 2:
                seen.append("erased")
                continue
            dep_j = shifted_depth(uv_i, depth, marg_R, marg_P, new_R, new_P)
            if f.obs[0][7] > 0:
                f.estimated_depth, f.lidar_depth_flag = f.obs[0][7], True
                seen.append("lidar")
            elif dep_j > 0:
                f.estimated_depth, f.lidar_depth_flag = dep_j, False
                seen.append("dep_j")
            else:
                f.estimated_depth, f.lidar_depth_flag = self.init_depth, False
                seen.append("init")
            kept.append(f)
        self.feature = kept
        return seen

    def remove_back(self):
        """:341-357"""
        kept, seen = [], []
        for f in self.feature:
            if f.start_frame != 0:
                f.start_frame -= 1
            else:
                del f.obs[0]
                if len(f.obs) == 0:
                    seen.append("erased")
                    continue
            kept.append(f)
        self.feature = kept
        return seen

    def remove_front(self, frame_count):
        """:359-379; an index outside the observations (undefined there) leaves the feature as it is"""
        kept, seen = [], []
        for f in self.feature:
            if f.start_frame == frame_count:
                f.start_frame -= 1
                seen.append("newest")
            else:
                j = WINDOW - 1 - f.start_frame
                if f.end_frame() < frame_count - 1:
                    seen.append("skipped")
                elif 0 <= j < len(f.obs):
                    del f.obs[j]
                    if len(f.obs) == 0:
                        seen.append("erased")
                        continue
                    seen.append("cut")
            kept.append(f)
        self.feature = kept
        return seen

    def projections(self, mode, estimate_td=True, ids=None):
        """estimator.cpp:745-789 (MODE_WINDOW) and :849-889 (MODE_MARG_OLD) -> dict(records, inv_dep, lidar_flags)"""
        pose, ex, td, feat = ids if ids is not None else (ID_POSE, ID_EX, ID_TD if estimate_td else -1, ID_FEATURE)
        recs, feature_index = [], -1
        for f in self.feature:
            if not eligible(len(f.obs), f.start_frame):
                continue
            feature_index += 1
            imu_i = f.start_frame
            if mode == MODE_MARG_OLD and imu_i != 0:
                continue
            o0 = f.obs[0]
            for k, o in enumerate(f.obs):
                if k == 0:
                    continue
                recs.append(dict(pose_i=pose + imu_i, pose_j=pose + imu_i + k, ex=ex, feature=feat + feature_index, td=td, reserved=0, pts_i=o0[:3], pts_j=o[:3],
                                 velocity_i=o0[5:7], velocity_j=o[5:7], td_i=o0[8], td_j=o[8], row_i=o0[4], row_j=o[4]))
        return dict(records=recs, inv_dep=self.depth_vector(), lidar_flags=[int(f.lidar_depth_flag) for f in self._eligible()])


def records_array(recs, dtype):
    a = np.zeros(len(recs), dtype)
    for k, r in enumerate(recs):
        for key, v in r.items():
            a[k][key] = v
    return a


def table_array(fm, dtype):
    """the list as an array of fman.FEATURE_DTYPE, unused observations zero"""
    a = np.zeros(len(fm.feature), dtype)
    for k, f in enumerate(fm.feature):
        a[k]["feature_id"], a[k]["start_frame"], a[k]["n_obs"] = f.feature_id, f.start_frame, len(f.obs)
        a[k]["lidar_depth_flag"], a[k]["solve_flag"], a[k]["estimated_depth"] = int(f.lidar_depth_flag), f.solve_flag, f.estimated_depth
        for j, o in enumerate(f.obs):
            a[k]["obs"][j] = (o[0:3], o[3:5], o[5:7], o[7], o[8])
    return a


def same_table(got, want):
    """bit equality of two FEATURE_DTYPE arrays over everything that is defined: the header and the first n_obs observations
    -> None, or a description of the first difference"""
    if len(got) != len(want):
        return f"{len(got)} features, expected {len(want)}"
    for k in range(len(want)):
        g, w = got[k], want[k]
        for key in ("feature_id", "start_frame", "n_obs", "lidar_depth_flag", "solve_flag"):
            if g[key] != w[key]:
                return f"feature {k} (id {w['feature_id']}): {key} {g[key]}, expected {w[key]}"
        if np.float64(g["estimated_depth"]).tobytes() != np.float64(w["estimated_depth"]).tobytes():
            return f"feature {k} (id {w['feature_id']}): estimated_depth {g['estimated_depth']!r}, expected {w['estimated_depth']!r}"
        n = int(w["n_obs"])
        if g["obs"][:n].tobytes() != w["obs"][:n].tobytes():
            return f"feature {k} (id {w['feature_id']}): observations differ"
    return None


# ---- scenes ---------------------------------------------------------------------------------------------------------
def quat_to_rot(q):
    """x y z w -> the rotation matrix, as Eigen's toRotationMatrix of the normalised quaternion"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rot_to_quat(R):
    """the rotation matrix -> x y z w (w > 0 for the small rotations of the scenes)"""
    w = math.sqrt(max(0.0, 1.0 + R[0][0] + R[1][1] + R[2][2])) / 2.0
    return np.array([(R[2][1] - R[1][2]) / (4 * w), (R[0][2] - R[2][0]) / (4 * w), (R[1][0] - R[0][1]) / (4 * w), w])


def slide_old_frames(back_R0, back_P0, Rs0, Ps0, ric, tic):
    """R0, P0, R1, P1 of slideWindowOld (estimator.cpp:1089-1094), every entry (t0 + t1) + t2"""
    back_R0, Rs0, ric = _mat(back_R0), _mat(Rs0), _mat(ric)
    tic = [float(v) for v in tic]
    a, b = mul3v(back_R0, tic), mul3v(Rs0, tic)
    return mul33(back_R0, ric), [float(back_P0[k]) + a[k] for k in range(3)], mul33(Rs0, ric), [float(Ps0[k]) + b[k] for k in range(3)]


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


RIC = rot([0.2, -0.5, 0.8], 0.05)
TIC = np.array([0.05, -0.02, 0.03])


def trajectory(rs, frames, step=0.08):
    """body poses: `step` metres per frame mostly sideways, a slow turn"""
    Ps, Rs = np.zeros((frames, 3)), np.zeros((frames, 3, 3))
    p, R = np.array([0.3, -0.2, 0.1]), rot([0.1, 0.3, -0.2], 0.1)
    for i in range(frames):
        Ps[i], Rs[i] = p, R
        d = np.array([1.0, 0.25 * rs.uniform(-1, 1), 0.15 * rs.uniform(-1, 1)])
        p = p + R @ (step * d / np.linalg.norm(d))
        R = R @ rot(rs.normal(0, 1, 3), 0.01)
    return Ps, Rs


def _camera(Ps, Rs, i):
    return Rs[i] @ RIC, Ps[i] + Rs[i] @ TIC


def observe(Pw, Ps, Rs, i, rs, noise):
    """-> the 8 doubles of the tracker's message for world point Pw in frame i, lidar depth -1"""
    Rc, tc = _camera(Ps, Rs, i)
    pc = Rc.T @ (Pw - tc)
    x, y = pc[0] / pc[2] + noise * rs.normal(), pc[1] / pc[2] + noise * rs.normal()
    return [x, y, 1.0, FOCAL * x + 320.0, FOCAL * y + 240.0, rs.normal(0, 0.05), rs.normal(0, 0.05), -1.0]


def window_scene(seed, n_features, noise=1.0 / FOCAL, lidar_share=0.0, starts=None, lengths=None, behind=None, still=0, lidar_of=None):
    """an 11-frame window: 8 cm steps, depths 2..20 m, pixel noise, 2..11 observations per feature.
    starts, lengths: taken in turn instead of drawn; lidar_of(fid, o): observation o carries a lidar depth; behind(fid): the point lies behind the start camera (a negative depth);
    still: the first `still` frames share one pose.
    -> dict(Ps, Rs, tic, ric, frames: per frame (ids, obs [n][8]), depth: id -> the constructed depth in the start frame)"""
    rs = np.random.RandomState(seed)
    Ps, Rs = trajectory(rs, MAX_OBS)
    for i in range(1, still):
        Ps[i], Rs[i] = Ps[0], Rs[0]
    frames = [([], []) for _ in range(MAX_OBS)]
    depth = {}
    for fid in range(n_features):
        start = int(starts[fid % len(starts)]) if starts is not None else int(rs.randint(0, WINDOW - 2))
        k = int(lengths[fid % len(lengths)]) if lengths is not None else int(rs.randint(2, MAX_OBS + 1))
        k = min(k, MAX_OBS - start)
        Rc, tc = _camera(Ps, Rs, start)
        z = rs.uniform(2.0, 20.0)
        if behind is not None and behind(fid):
            z = -z
        Pw = Rc @ (z * np.array([rs.uniform(-0.5, 0.5), rs.uniform(-0.4, 0.4), 1.0])) + tc
        depth[fid] = z
        lidar_at = int(rs.randint(0, k)) if rs.uniform() < lidar_share else -1
        for o in range(k):
            ob = observe(Pw, Ps, Rs, start + o, rs, noise)
            if o == lidar_at or (lidar_of is not None and lidar_of(fid, o)):
                Rj, tj = _camera(Ps, Rs, start + o)
                ob[7] = float((Rj.T @ (Pw - tj))[2])
            frames[start + o][0].append(fid)
            frames[start + o][1].append(ob)
    return dict(Ps=Ps, Rs=Rs, tic=TIC.copy(), ric=RIC.copy(), frames=frames, depth=depth)


def sequence(seed, n_frames=14, per_frame=60, lidar_share=0.3, still=(), step=0.08):
    """a tracker's output over n_frames images: every frame keeps most of its features and tops up to per_frame new ones;
    frames listed in `still` do not move (so their parallax is below the keyframe threshold).
    -> dict(Ps, Rs [n_frames], frames: per image (ids, obs [n][8]))"""
    rs = np.random.RandomState(seed)
    Ps, Rs = trajectory(rs, n_frames, step)
    for i in range(1, n_frames):
        if i in still:
            shift = Ps[i] - Ps[i - 1]
            Ps[i:] -= shift
            Rs[i] = Rs[i - 1]
    alive, next_id, frames = {}, 0, []
    for i in range(n_frames):
        Rc, tc = _camera(Ps, Rs, i)
        alive = {fid: Pw for fid, Pw in alive.items() if rs.uniform() < 0.9}
        while len(alive) < per_frame:
            z = rs.uniform(2.0, 20.0)
            alive[next_id] = Rc @ (z * np.array([rs.uniform(-0.5, 0.5), rs.uniform(-0.4, 0.4), 1.0])) + tc
            next_id += 1
        ids, obs = [], []
        for fid in sorted(alive):
            ob = observe(alive[fid], Ps, Rs, i, rs, 0.3 / FOCAL)
            if rs.uniform() < lidar_share * 0.3:
                ob[7] = float((Rc.T @ (alive[fid] - tc))[2])
            ids.append(fid)
            obs.append(ob)
        frames.append((ids, obs))
    return dict(Ps=Ps, Rs=Rs, tic=TIC.copy(), ric=RIC.copy(), frames=frames)


def load(fm, frames, td=0.0, first=0):
    """feed per-frame (ids, obs) into a manager (reference or device binding alike) -> the add_frame results"""
    return [fm.add_frame(first + i, ids, np.asarray(obs, np.float64).reshape(-1, 8), td) for i, (ids, obs) in enumerate(frames)]


# ---- the triangulation scenes of both tiers ----------------------------------------------------------------------------
SLOT_TARGET = 300


def _tri_scene(name):
    if name == "main":            # the issue's window: 400 features, 2..11 observations
        return window_scene(11, 400)
    if name == "shapes":          # 2, 3 and 11 (as many as fit) observations from start_frame 0, 7 and 8 (8 is skipped)
        return window_scene(21, 27, starts=[0, 0, 0, 7, 7, 7, 8, 8, 8], lengths=[2, 3, 11] * 3)
    if name == "sign":            # odd ids lie behind the camera: depth <= -2; even ids in front
        return window_scene(31, 40, behind=lambda fid: fid % 2 == 1)
    if name == "slot":            # feature SLOT_TARGET starts last and has the largest id: slot 300 of the table
        return window_scene(41, SLOT_TARGET + 1, starts=[k % 8 for k in range(SLOT_TARGET)] + [7], lengths=[2 + k % 10 for k in range(SLOT_TARGET)] + [3])
    if name == "still":           # frames 0..2 share one pose and there is no noise: features that end there have rank 2 (gap 0)
        return window_scene(51, 30, noise=0.0, starts=[0, 0, 3, 1], lengths=[3, 2, 5, 6], still=3)
    raise KeyError(name)


TRI_SCENES = ("main", "shapes", "sign", "slot", "still")
_tri_cache = {}


def tri_reference(name):
    """-> dict(scene, fm: the loaded reference manager before triangulate, ids, numpy, exact (mpf), G, gaps): the features
    triangulate works on, their float64 (numpy) and mpmath depths, G = the largest relative deviation of the two ON THAT
    SCENE, and (sigma_3 - sigma_4) / sigma_1 per feature.  Computed once per process."""
    if name not in _tri_cache:
        sc = _tri_scene(name)
        fm = FeatureManager()
        load(fm, sc["frames"])
        ids, dn, de, gaps = [], [], [], []
        for f in fm.to_triangulate():
            d, sv = depth_numpy(sc["Ps"], sc["Rs"], sc["tic"], sc["ric"], f.start_frame, f.obs)
            ids.append(f.feature_id)
            dn.append(d)
            de.append(depth_mp(sc["Ps"], sc["Rs"], sc["tic"], sc["ric"], f.start_frame, f.obs))
            gaps.append(float((sv[2] - sv[3]) / sv[0]))
        ok = [k for k in range(len(ids)) if gaps[k] >= 1e-6]             # G is not defined where the null space is not a line
        G = max([rel_dev(dn[k], de[k]) for k in ok], default=0.0)
        _tri_cache[name] = dict(scene=sc, fm=fm, ids=ids, numpy=dn, exact=de, G=G, gaps=gaps)
    return _tri_cache[name]


def tri_bar(G):
    """10 x G, the project's margin over the reference's own spread, and never below 16 ulp"""
    return max(10.0 * G, 16 * 2.0 ** -52)
