"""GPU tier of the feature table (include/lvi_fman.h) against tests/fman_ref.py.

Every figure is printed before it is asserted.  Everything except the triangulated depth is copies, comparisons and
correctly rounded + - * / sqrt in a stated order: the device table after every operation equals the reference's BIT FOR BIT
(ids, start_frame, counts, flags, every observation double, estimated_depth after the shift, parallax_sum, the keyframe
decision, last_track_num, the emitted records and their order, the correspondences).  The triangulated depth is compared with
mpmath: the bar is 10 G, G being the largest relative deviation of the float64 numpy SVD from mpmath on that scene, and never
below 16 ulp (fman_ref.tri_bar).  Measured on the MI355X, scene `main` (400 features): G 2.1e-13, device worst 5.0e-14,
median 1.1e-15 (DESIGN §26 has every scene)."""
import numpy as np
import pytest

import fman_ref as R

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.float64(x).tobytes()


def _same(tab, fm, what):
    diff = R.same_table(tab.download(), R.table_array(fm, tab.feature_dtype))
    assert diff is None, f"{what}: {diff}"
    assert tab.count() == (len(fm.feature), fm.get_feature_count()), what


def _same_info(got, want, what):
    print(f"[fman gpu] {what}: device {got}")
    for k in ("last_track_num", "parallax_num", "keyframe", "added"):
        assert got[k] == want[k], (what, k, got, want)
    assert _bits(got["parallax_sum"]) == _bits(want["parallax_sum"]), (what, got, want)


def _frame(rs, ids, lidar_share=0.3, spread=1.0):
    """a tracker message for `ids`: points around (0.1 id mod 7, ...) moved by `spread`"""
    obs = np.zeros((len(ids), 8))
    for k, i in enumerate(ids):
        x, y = 0.1 * (i % 7) - 0.3 + spread * rs.normal(0, 0.03), 0.08 * (i % 5) - 0.16 + spread * rs.normal(0, 0.03)
        obs[k] = [x, y, 1.0, 460 * x + 320, 460 * y + 240, rs.normal(0, 0.1), rs.normal(0, 0.1), rs.uniform(2, 20) if rs.uniform() < lidar_share else -1.0]
    return obs


@pytest.fixture(scope="module")
def tab(pkg, hip):
    t = pkg.FeatureTable(hip, max_features=2100)
    yield t
    t.close()


def _fresh(tab):
    tab.clear()
    assert tab.count() == (0, 0) and len(tab.download()) == 0
    return R.FeatureManager()


def _load(tab, fm, frames, td=0.0):
    for i, (ids, obs) in enumerate(frames):
        o = np.asarray(obs, np.float64).reshape(-1, 8)
        got, want = tab.add_frame(i, ids, o, td), fm.add_frame(i, ids, o, td)
        assert (got["last_track_num"], got["added"], got["keyframe"], got["parallax_num"]) == \
            (want["last_track_num"], want["added"], want["keyframe"], want["parallax_num"]) and _bits(got["parallax_sum"]) == _bits(want["parallax_sum"]), (i, got, want)


# ---- addFeatureCheckParallax ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1025])
def test_add_frame_tables(tab, n):
    """tables of 0..1025 features (wavefront and scan-round edges): a first frame, matched and unmatched ids alternating, then
    three fully tracked frames.  The parallax is taken between frame_count - 2 and frame_count - 1: frame 2 repeats frame 1 and
    frame 3 moves, so image 3 decides "no keyframe" and image 4 "keyframe".  Small tables take the early `true` (last_track_num
    < 20), frames 0 and 1 the one of frame_count < 2; the lidar depth arrives on the first, on a later and on no observation"""
    rs = np.random.RandomState(100 + n)
    fm = _fresh(tab)
    even = list(range(0, 2 * n, 2))
    every = list(range(0, 2 * n + 1))
    script = [(0, even, 1.0, "first frame"), (1, every, 1.0, "matched and unmatched alternating"), (2, every, 0.0, "tracked, still"),
              (3, every, 3.0, "tracked, moving"), (4, every, 1.0, "tracked")]
    keys = []
    for fc, ids, spread, what in script:
        if fc == 2:
            obs = np.array([o[-1][:8] for o in (f.obs for f in fm.feature)])       # the same points again: no parallax
            obs[:, 7] = np.where(rs.uniform(size=len(obs)) < 0.2, 7.5, -1.0)       # a lidar depth arriving late
            order = np.argsort([f.feature_id for f in fm.feature])
            obs = obs[order]
        else:
            obs = _frame(rs, ids, spread=spread)
        got, want = tab.add_frame(fc, ids, obs, 0.01 * fc), fm.add_frame(fc, ids, obs, 0.01 * fc)
        _same_info(got, want, f"table {n}, {what}")
        _same(tab, fm, f"table {n}, {what}")
        keys.append((got["keyframe"], got["parallax_num"]))
    assert len(fm.feature) == 2 * n + 1
    if n >= 63:
        # frames 0 | 1: the n features of the first frame; 1 | 2: no motion; 2 | 3: motion.  Both decisions, every feature summed
        assert keys[:2] == [(1, 0), (1, 0)] and keys[2][1] == n and keys[3] == (0, 2 * n + 1) and keys[4] == (1, 2 * n + 1), keys
        late = [f for f in fm.feature if f.lidar_depth_flag and f.obs[0][7] == 7.5]
        never = [f for f in fm.feature if not f.lidar_depth_flag]
        first = [f for f in fm.feature if f.lidar_depth_flag and f.obs[0][7] != 7.5]
        print(f"[fman gpu] table {n}: lidar depth on the first observation {len(first)}, on a later one {len(late)}, on none {len(never)}")
        assert late and never and first
    else:
        assert all(k == (1, 0) for k in keys), keys                                # last_track_num < 20: the early `true`


@pytest.mark.parametrize("n", [0, 1, 150])
def test_frames_of_0_1_and_150_on_a_table_of_257(tab, n):
    rs = np.random.RandomState(7 + n)
    fm = _fresh(tab)
    _load(tab, fm, [(list(range(257)), _frame(rs, range(257))), (list(range(257)), _frame(rs, range(257)))])
    ids = list(range(100, 100 + 2 * n, 2))[:n // 2] + list(range(1000, 1000 + n - n // 2))     # half known, half new
    obs = _frame(rs, ids, spread=2.0)
    got, want = tab.add_frame(2, ids, obs, -0.02), fm.add_frame(2, ids, obs, -0.02)
    _same_info(got, want, f"frame of {n}")
    _same(tab, fm, f"frame of {n}")
    assert got["added"] == n - n // 2 and got["last_track_num"] == n // 2


def test_errors_leave_the_state_unchanged(pkg, hip):
    E = pkg._abi
    t = pkg.FeatureTable(hip, max_features=100)
    try:
        rs = np.random.RandomState(3)
        fm = R.FeatureManager()
        _load(t, fm, [(list(range(90)), _frame(rs, range(90)))])
        before = t.download().tobytes()
        with pytest.raises(pkg.LviError) as e:                                     # 90 + 11 > 100
            t.add_frame(1, list(range(80, 101)), _frame(rs, range(80, 101)))
        assert e.value.code == E.LVI_ERR_CAPACITY
        with pytest.raises(pkg.LviError) as e:                                     # a std::map has no such order
            t.add_frame(1, [5, 4], _frame(rs, [5, 4]))
        assert e.value.code == E.LVI_ERR_INVALID_ARG
        with pytest.raises(pkg.LviError) as e:
            t.add_frame(11, [5], _frame(rs, [5]))
        assert e.value.code == E.LVI_ERR_INVALID_ARG
        with pytest.raises(pkg.LviError) as e:
            t.set_depth(np.ones(3))                                                # getFeatureCount() is 0
        assert e.value.code == E.LVI_ERR_INVALID_ARG
        assert t.download().tobytes() == before and t.count() == (90, 0)
        ids = list(range(80, 90)) + [200 + k for k in range(10)]                   # 10 known, 10 new: exactly full
        obs = _frame(rs, ids)
        _same_info(t.add_frame(1, ids, obs, 0.0), fm.add_frame(1, ids, obs, 0.0), "the frame that fits")
        _same(t, fm, "after the refused frames")
        assert t.count()[0] == 100
    finally:
        t.close()


# ---- depth vector, setDepth, removeFailures, clearDepth, the emission, getCorresponding -----------------------------
SLIDE_STARTS, SLIDE_LENGTHS = [0, 1, 2, 3, 5, 7, 8, 9, 9, 10], [2, 11, 3, 1, 5, 9, 4]


def _lidar_pattern(fid):
    return (fid // 10) % 4                                  # 0: no lidar depth, 1: on observation 0, 2: on observation 1, 3: on every one


def _slide_scene(n):
    """every pair of SLIDE_STARTS x SLIDE_LENGTHS with every lidar pattern: each branch of the slides occurs from 65 features on"""
    return R.window_scene(60 + n, n, starts=SLIDE_STARTS, lengths=SLIDE_LENGTHS,
                          lidar_of=lambda fid, o: _lidar_pattern(fid) == 3 or (_lidar_pattern(fid) == 1 and o == 0) or (_lidar_pattern(fid) == 2 and o == 1))


@pytest.mark.parametrize("n", [65, 1025])
def test_depths_failures_records_and_correspondences(tab, n):
    sc = _slide_scene(n)
    fm = _fresh(tab)
    _load(tab, fm, sc["frames"], td=0.003)
    dep = tab.depth_vector()
    assert dep.tobytes() == np.array(fm.depth_vector()).tobytes() and len(dep) == fm.get_feature_count() > 0
    rs = np.random.RandomState(n)
    for td in (True, False):
        for mode in (R.MODE_WINDOW, R.MODE_MARG_OLD):
            got, want = tab.projections(mode, estimate_td=td), fm.projections(mode, estimate_td=td)
            print(f"[fman gpu] table {n}, mode {mode}, td {td}: {len(got['records'])} records over {len(got['inv_dep'])} features")
            assert got["records"].tobytes() == R.records_array(want["records"], tab.record_dtype).tobytes()
            assert got["inv_dep"].tobytes() == np.array(want["inv_dep"]).tobytes() and list(got["lidar_flags"]) == want["lidar_flags"]
            assert len(got["inv_dep"]) == fm.get_feature_count()
    assert 0 < len(tab.projections(R.MODE_MARG_OLD)["records"]) < len(tab.projections(R.MODE_WINDOW)["records"])
    for l, r in ((0, 10), (3, 5), (9, 10), (5, 3), (4, 4)):
        got, want = tab.corresponding(l, r), np.array(fm.corresponding(l, r), np.float64).reshape(-1, 2, 3)
        print(f"[fman gpu] table {n}: {len(got)} correspondences of frames {l}, {r}")
        assert got.tobytes() == want.tobytes() and (len(got) > 0 or (l, r) == (0, 10) and n < 100)
    x = dep * np.where(rs.uniform(size=len(dep)) < 0.3, -1.0, 1.0) * rs.uniform(0.5, 2.0, len(dep))
    tab.clear_depth(x)
    fm.clear_depth(x)
    _same(tab, fm, "clearDepth")
    assert not any(f.lidar_depth_flag for f in fm._eligible())
    tab.set_depth(x)
    fm.set_depth(x)
    _same(tab, fm, "setDepth with negative values")
    flags = [f.solve_flag for f in fm.feature]
    assert 2 in flags and 1 in flags and 0 in flags
    tab.remove_failures()
    fm.remove_failures()
    _same(tab, fm, "removeFailures")
    assert len(fm.feature) == len(flags) - flags.count(2)


# ---- the slides ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 257, 1025])
def test_slides(tab, n):
    """every branch of removeBackShiftDepth, removeBack and removeFront, the erasures included"""
    sc = _slide_scene(n)
    margR, newR = R.rot([0.3, -0.1, 0.2], 0.2), R.rot([0.1, 0.2, -0.3], 0.25)
    margP, newP = np.array([0.4, -0.3, 0.2]), np.array([0.7, -0.2, 0.25])
    for op in ("back_shift", "back", "front", "front_9"):
        fm = _fresh(tab)
        _load(tab, fm, sc["frames"])
        if op == "back_shift":
            x = np.array(fm.depth_vector()) * np.array([-1.0 if _lidar_pattern(f.feature_id) == 0 else 1.0 for f in fm._eligible()])   # a failed solve and no lidar
            tab.set_depth(x)
            fm.set_depth(x)
            tab.remove_back_shift_depth(margR, margP, newR, newP)
            seen = fm.remove_back_shift_depth(margR, margP, newR, newP)
            need = {"shifted", "erased", "lidar", "dep_j", "init"}
        elif op == "back":
            tab.remove_back()
            seen, need = fm.remove_back(), {"erased"}
        else:
            fc = 10 if op == "front" else 9
            tab.remove_front(fc)
            # with frame_count 9 nothing can be erased (a single observation at frame 9 is the `newest` branch), and the feature
            # whose last frame is 8 names an observation it does not have: left as it is
            seen, need = fm.remove_front(fc), {"newest", "skipped", "cut"} | ({"erased"} if fc == 10 else set())
        print(f"[fman gpu] table {n}, {op}: {len(fm.feature)} features left; outcomes {sorted(set(seen))}")
        _same(tab, fm, f"table {n}, {op}")
        assert need <= set(seen), (op, set(seen))
        # a second slide on the compacted table (it now lies in the other buffer)
        tab.remove_back()
        fm.remove_back()
        _same(tab, fm, f"table {n}, {op}, then removeBack")


# ---- triangulate ---------------------------------------------------------------------------------------------------
def _triangulated(tab, name, keep=None):
    """load scene `name` (only the ids of `keep`, if given), triangulate -> (id -> (slot, feature), info, the table before, after)"""
    r = R.tri_reference(name)
    sc = r["scene"]
    frames = sc["frames"]
    if keep is not None:
        frames = [([i for i in ids if i in keep], [o for i, o in zip(ids, obs) if i in keep]) for ids, obs in frames]
    fm = _fresh(tab)
    _load(tab, fm, frames)
    before = tab.download()
    info = tab.triangulate(sc["Ps"], sc["Rs"], sc["tic"], sc["ric"])
    after = tab.download()
    return {int(f["feature_id"]): (k, f) for k, f in enumerate(after)}, info, before, after


@pytest.mark.parametrize("name", ["main", "shapes", "sign", "slot"])
def test_triangulated_depth_against_mpmath(tab, name):
    r = R.tri_reference(name)
    by_id, info, before, after = _triangulated(tab, name)
    bar = R.tri_bar(r["G"])
    dev, negative = [], 0
    for k, fid in enumerate(r["ids"]):
        d = float(by_id[fid][1]["estimated_depth"])
        if r["exact"][k] < 0:
            negative += 1
            assert abs(r["exact"][k]) >= 1 and d == R.INIT_DEPTH, (fid, d, r["exact"][k])      # depth < 0 becomes init_depth exactly
        else:
            assert r["exact"][k] >= 1 and d != R.INIT_DEPTH
            dev.append(R.rel_dev(d, r["exact"][k]))
    print(f"[fman gpu] scene {name}: {len(r['ids'])} triangulated ({negative} negative), G {r['G']:.3e}, bar {bar:.3e}, device worst {max(dev):.3e}, "
          f"median {np.median(dev):.3e}, most sweeps {info['max_sweeps']}")
    assert info["triangulated"] == len(r["ids"]) and info["negative"] == negative and info["non_finite"] == 0 and 1 <= info["max_sweeps"] < 30
    assert max(dev) <= bar
    # nothing else moved: every other field, and the depth of every feature the skip rule passes over
    touched = set(r["ids"])
    b2 = before.copy()
    for k in range(len(b2)):
        if int(b2[k]["feature_id"]) in touched:
            b2[k]["estimated_depth"] = after[k]["estimated_depth"]
    assert R.same_table(after, b2) is None
    if name == "sign":
        assert negative == 20
    if name == "shapes":
        assert any(int(f["start_frame"]) == 8 and f["estimated_depth"] == -1.0 for f in after)      # start_frame 8 is skipped
    if name == "main":
        assert min(r["gaps"]) >= 1e-2                                             # the scene condition, no feature excluded


def test_triangulation_does_not_depend_on_slot_or_run(tab):
    by_id, _, _, after = _triangulated(tab, "slot")
    slot, f300 = by_id[R.SLOT_TARGET]
    again = _triangulated(tab, "slot")[3]
    alone, _, _, _ = _triangulated(tab, "slot", keep={R.SLOT_TARGET})
    print(f"[fman gpu] feature {R.SLOT_TARGET}: slot {slot} depth {float(f300['estimated_depth'])!r}; slot {alone[R.SLOT_TARGET][0]} depth "
          f"{float(alone[R.SLOT_TARGET][1]['estimated_depth'])!r}")
    assert slot == 300 and alone[R.SLOT_TARGET][0] == 0
    assert _bits(f300["estimated_depth"]) == _bits(alone[R.SLOT_TARGET][1]["estimated_depth"])
    assert R.same_table(again, after) is None                                      # two runs, the same bits


def test_pure_rotation_feature_leaves_the_others_alone(tab):
    r = R.tri_reference("still")
    flat = {fid for k, fid in enumerate(r["ids"]) if r["gaps"][k] < 1e-12}
    rest = set(r["ids"]) - flat
    by_id, info, _, _ = _triangulated(tab, "still")
    without, _, _, _ = _triangulated(tab, "still", keep=rest)
    vals = [float(by_id[i][1]["estimated_depth"]) for i in sorted(flat)]
    print(f"[fman gpu] {len(flat)} features without a baseline: depths {vals[:6]} ..., non_finite {info['non_finite']}, most sweeps {info['max_sweeps']}")
    assert len(flat) >= 8 and all(np.isfinite(v) or np.isnan(v) for v in vals)
    for i in rest:
        assert _bits(by_id[i][1]["estimated_depth"]) == _bits(without[i][1]["estimated_depth"]), i
    bar = R.tri_bar(r["G"])
    dev = [R.rel_dev(float(by_id[fid][1]["estimated_depth"]), r["exact"][k]) for k, fid in enumerate(r["ids"]) if fid in rest]
    print(f"[fman gpu] scene still: G {r['G']:.3e}, bar {bar:.3e}, device worst {max(dev):.3e}")
    assert max(dev) <= bar


# ---- the host mirror and the chain ---------------------------------------------------------------------------------
CHAIN_SEED, CHAIN_STILL = 6, (10, 12)


def test_host_mirror_equals_the_direct_abi(pkg, hip, tab):
    H = pkg.host_api
    seq = R.sequence(CHAIN_SEED, n_frames=3, per_frame=60, step=0.3)
    FM = H.FeatureManager(pkg.load_host(), hip, max_features=256)
    try:
        fm = _fresh(tab)
        for i, (ids, obs) in enumerate(seq["frames"]):
            a, b = FM.add_frame(i, ids, obs, 0.004), tab.add_frame(i, ids, np.asarray(obs), 0.004)
            _same_info(a, b, f"host mirror frame {i}")
            _same_info(a, fm.add_frame(i, ids, obs, 0.004), f"host mirror frame {i} against the reference")
            assert R.same_table(FM.table.download(), tab.download()) is None
        assert FM.table.count() == tab.count() and tab.count()[1] > 0
    finally:
        FM.close()


def test_chain_of_14_frames(pkg, hip):
    """add_frame; from frame_count == 10 on triangulate, fillWindow, VinsWindowOptimizer::optimize, takeDepths, VinsMarginalizer,
    the slide the keyframe decision asks for, removeFailures.  The reference is driven beside it with the DEVICE's solved depths
    and poses (and its triangulated depths), so the table parity stays bit for bit."""
    H = pkg.host_api
    hl = pkg.load_host()
    seq = R.sequence(CHAIN_SEED, n_frames=14, per_frame=60, still=CHAIN_STILL, step=0.3)
    rs = np.random.RandomState(1)
    tic, ric, td = seq["tic"], seq["ric"], 0.002
    ex = np.r_[tic, R.rot_to_quat(ric)]

    def guess(i):                                          # the pose a front end would hand in: the truth, slightly off
        return np.r_[seq["Ps"][i] + rs.normal(0, 0.005, 3), R.rot_to_quat(seq["Rs"][i] @ R.rot(rs.normal(0, 1, 3), 0.002))]

    FM = H.FeatureManager(hl, hip, max_features=512)
    V = H.VinsMarginalizer(hl, hip, max_features=200, estimate_td=True)
    O = H.VinsWindowOptimizer(hl, hip, V, max_features=200, estimate_extrinsic=0, num_iterations=8, solver_time=0.0)
    fm, poses, slides, frame_count = R.FeatureManager(), [], [], 0
    try:
        for i, (ids, obs) in enumerate(seq["frames"]):
            poses.append(guess(i))
            info = FM.add_frame(frame_count, ids, obs, td)
            _same_info(info, fm.add_frame(frame_count, ids, obs, td), f"chain image {i}")
            _same(FM.table, fm, f"chain image {i}, add_frame")
            if frame_count < R.WINDOW:
                frame_count += 1
                continue
            assert len(poses) == R.MAX_OBS
            Ps = np.array([p[:3] for p in poses])
            Rs = np.array([R.quat_to_rot(p[3:]) for p in poses])
            want = {f.feature_id for f in fm.to_triangulate()}
            tri = FM.triangulate(Ps, Rs, tic, ric)
            got = {int(f["feature_id"]): float(f["estimated_depth"]) for f in FM.table.download()}
            assert tri["triangulated"] == len(want) and tri["non_finite"] == 0
            fm.triangulate(Ps, Rs, tic, ric, depth_of=lambda f: got[f.feature_id])       # the device's depths (the sign rule is idempotent)
            _same(FM.table, fm, f"chain image {i}, triangulate")
            flag = V.MARGIN_OLD if info["keyframe"] else V.MARGIN_SECOND_NEW
            V.set_window(np.array(poses), np.zeros((11, 9)), ex, td)
            FM.fill_window(V, O)
            sol = O.optimize(flag)
            out = O.window()
            print(f"[fman gpu] chain image {i}: {len(fm.feature)} features, {fm.get_feature_count()} in the solve, {len(want)} triangulated; solve status "
                  f"{sol['status']}, cost {sol['initial_cost']:.4g} -> {sol['final_cost']:.4g} in {sol['iterations']} iterations; flag {flag}")
            assert len(out["inv_dep"]) == len(fm.feature)
            FM.take_depths(V)
            fm.set_depth([out["inv_dep"][k] for k, f in enumerate(fm.feature) if R.eligible(len(f.obs), f.start_frame)])
            _same(FM.table, fm, f"chain image {i}, takeDepths")
            poses = [out["pose"][k].copy() for k in range(R.MAX_OBS)]
            V.set_imu(0.0)
            ran = V.run(flag)
            print(f"[fman gpu] chain image {i}: marginalisation ran {ran['ran']}, status {ran['status']}, m {ran['m']}, n {ran['n']}")
            if flag == V.MARGIN_OLD:
                back_R0, back_P0, Rs0, Ps0 = R.quat_to_rot(poses[0][3:]), poses[0][:3], R.quat_to_rot(poses[1][3:]), poses[1][:3]
                FM.slide_old(True, back_R0, back_P0, Rs0, Ps0, ric, tic)
                seen = fm.remove_back_shift_depth(*R.slide_old_frames(back_R0, back_P0, Rs0, Ps0, ric, tic))
                del poses[0]
            else:
                FM.slide_new(frame_count)
                seen = fm.remove_front(frame_count)
                del poses[R.WINDOW - 1]
            slides.append(flag)
            _same(FM.table, fm, f"chain image {i}, slide {sorted(set(seen))}")
            FM.remove_failures()
            fm.remove_failures()
            _same(FM.table, fm, f"chain image {i}, removeFailures")
        print(f"[fman gpu] chain: slides {slides}")
        assert len(slides) == 4 and V.MARGIN_OLD in slides and V.MARGIN_SECOND_NEW in slides
    finally:
        O.close()
        V.close()
        FM.close()
