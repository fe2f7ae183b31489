"""GPU tier (-m gpu) of the batched device RANSAC (include/lvi_fmatb.h).  The yardstick of every test is a separate
pkg.FundamentalRansac per slot given the same inputs (tests/test_gpu_fmat.py pins that handle to the host restatement): the
status bytes, every field of the info record but stream_us and every array of the trace must be the same bits, so no tolerance
appears here.  Scenes come from tests/fmat_ref.two_view."""
import ctypes as C

import numpy as np
import pytest

import fmat_ref as R

pytestmark = pytest.mark.gpu

THRESHOLDS = (1.0, 0.5, 3.0)
MAX_POINTS = 1000


def _b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _scene(n, seed, kind="general", outliers=0.3):
    p1, p2, _, _ = R.two_view(n, outliers, 0.3 if kind == "general" else 0.0, seed=seed * 1000 + n, kind=kind)
    return p1, p2


def _exact_line(n):
    """n points exactly on a line in both views: getSubset never finds an acceptable subset"""
    k = np.arange(n)
    p1 = np.c_[50 + 8 * k, 100 + 2 * k].astype(np.float32)
    return p1, p1 + np.float32(3)


@pytest.fixture(scope="module")
def singles(pkg, hip):
    """one single handle per max_iters, made on first use"""
    made = {}

    def get(max_iters=1000):
        if max_iters not in made:
            made[max_iters] = pkg.FundamentalRansac(hip, max_points=MAX_POINTS, max_iters=max_iters)
        return made[max_iters]
    yield get
    for h in made.values():
        h.close()


def _assert_slot_equals_single(single, pair, thr, got, trace, tag):
    st_s, info_s = single.find(pair[0], pair[1], thr, with_info=True)
    tr_s = single.trace()
    st_b, info_b = got
    np.testing.assert_array_equal(st_b, st_s, err_msg=tag)
    for k in ("path", "iters", "n_subsets", "best_iter", "best_root", "n_inliers"):
        assert info_b[k] == info_s[k], (tag, k, info_b[k], info_s[k])
    np.testing.assert_array_equal(_b64(info_b["best_median"]), _b64(info_s["best_median"]), err_msg=tag)
    np.testing.assert_array_equal(_b64(info_b["F"]), _b64(info_s["F"]), err_msg=tag)
    assert info_b["stream_us"] >= 0
    for k in ("subsets", "nmodels", "score"):
        np.testing.assert_array_equal(trace[k], tr_s[k], err_msg=f"{tag} trace {k}")
    np.testing.assert_array_equal(_b64(trace["F"]), _b64(tr_s["F"]), err_msg=f"{tag} trace F")
    return info_s


def _check_call(batch, single, pairs, thr):
    out = batch.find(pairs, thr)
    infos = []
    for s, pr in enumerate(pairs):
        if pr is None:
            assert out[s] is None
            assert len(batch.trace(s)["subsets"]) == 0
            infos.append(None)
        else:
            infos.append(_assert_slot_equals_single(single, pr, thr[s], out[s], batch.trace(s), f"slot {s} n {len(pr[0])}"))
    return out, infos


# --------------------------------------------------------------------------------------------- 1. slot counts, mixed paths
CALLS = {
    1: [[("general", 150)], [("line", 40)], [("duplicates", 16)], [("collinear", 15)]],
    3: [[("general", 7), ("general", 14), ("general", 150)], [("line", 40), ("duplicates", 16), ("collinear", 15)]],
    8: [[("general", 7), ("general", 8), ("general", 14), ("general", 15), ("general", 16), ("general", 150), ("general", 1000), ("general", 150)],
        [("general", 16), ("line", 150), ("general", 8), ("duplicates", 150), ("collinear", 150), ("general", 7), ("duplicates", 14), ("general", 15)]],
}


@pytest.mark.parametrize("slots", (1, 3, 8))
def test_every_slot_equals_a_single_handle(pkg, hip, singles, slots):
    batch = pkg.FundamentalRansacBatch(hip, slots, max_points=MAX_POINTS)
    try:
        paths = set()
        for c, call in enumerate(CALLS[slots]):
            pairs = [_exact_line(n) if kind == "line" else _scene(n, 10 * slots + s + c, kind) for s, (kind, n) in enumerate(call)]
            thr = [THRESHOLDS[(s + c) % 3] for s in range(slots)]
            out, infos = _check_call(batch, singles(), pairs, thr)
            for s, (kind, n) in enumerate(call):
                paths.add(infos[s]["path"])
                if kind == "line":                               # no subset, no model, status zeros
                    assert infos[s]["n_subsets"] == 0 and infos[s]["best_iter"] == -1 and not out[s][0].any()
        assert paths == ({"ransac"} if slots == 1 else {"kernel", "lmeds", "ransac"})
    finally:
        batch.close()


# --------------------------------------------------------------------------------------------- 2. stale state
def _raw_find(pkg, batch, pairs, thr, status, infos=None):
    """lvi_fmatb_find on the caller's own status buffers (status[s]: uint8 array or None) -> the status code"""
    A = pkg._abi
    S = batch.slots
    keep = [None if pr is None else tuple(None if x is None else np.ascontiguousarray(x, np.float32) for x in pr[:2]) for pr in pairs]
    n = (C.c_int32 * S)(*[-1 if pr is None else int(pr[2]) if len(pr) > 2 else len(pr[0]) for pr in pairs])

    def table(arrs):
        return (C.c_void_p * S)(*[A._ptr(x) if x is not None else None for x in arrs])
    return batch.lib.dll.lvi_fmatb_find(batch._h, table([k and k[0] for k in keep]), table([k and k[1] for k in keep]), n, (C.c_double * S)(*thr), 0.99,
                                        table(status), infos)


def test_a_slot_that_sits_out_leaves_nothing_behind(pkg, hip, singles):
    S = 8
    batch = pkg.FundamentalRansacBatch(hip, S, max_points=MAX_POINTS)
    try:
        _check_call(batch, singles(), [_scene(150, 40 + s) for s in range(S)], [1.0] * S)
        ns = {0: 8, 2: 16, 3: 7, 5: 40, 7: 14}                   # slots 1, 4 and 6 sit out; the others on other paths and smaller
        pairs = [_scene(ns[s], 50 + s) if s in ns else None for s in range(S)]
        thr = [THRESHOLDS[s % 3] for s in range(S)]
        status = [np.full(150, 0xAB, np.uint8) for _ in range(S)]
        infos = (pkg.fmat.FmatInfo * S)()
        C.memset(infos, 0xAB, C.sizeof(infos))
        assert _raw_find(pkg, batch, pairs, thr, status, infos) == 0
        for s in range(S):
            if s in ns:
                got = (status[s][:ns[s]].copy(), pkg.fmat._info_dict(infos[s]))
                _assert_slot_equals_single(singles(), pairs[s], thr[s], got, batch.trace(s), f"slot {s}")
                assert (status[s][ns[s]:] == 0xAB).all()
            else:
                assert (status[s] == 0xAB).all()
                assert bytes(infos[s]) == bytes(C.sizeof(pkg.fmat.FmatInfo))
                assert all(len(v) == 0 for v in batch.trace(s).values())
    finally:
        batch.close()


# --------------------------------------------------------------------------------------------- 3. iteration limits
@pytest.mark.parametrize("max_iters", (1, 2))
def test_iteration_limits(pkg, hip, singles, max_iters):
    batch = pkg.FundamentalRansacBatch(hip, 4, max_points=MAX_POINTS, max_iters=max_iters)
    try:
        pairs = [_scene(16, 60), _scene(8, 61), _scene(150, 62), _scene(14, 63)]
        _, infos = _check_call(batch, singles(max_iters), pairs, [1.0, 1.0, 0.5, 3.0])
        assert [i["path"] for i in infos] == ["ransac", "lmeds", "ransac", "lmeds"]
        assert all(i["n_subsets"] <= max_iters for i in infos)
    finally:
        batch.close()


# --------------------------------------------------------------------------------------------- 4. errors are atomic
def test_errors_are_atomic(pkg, hip, singles):
    A = pkg._abi
    S = 8
    batch = pkg.FundamentalRansacBatch(hip, S, max_points=64)
    try:
        good = [_scene(20 + s, 70 + s) for s in range(S)]
        thr = [1.0] * S
        _check_call(batch, singles(), good, thr)
        before = [batch.trace(s) for s in range(S)]
        cnt = batch.counters()
        big = _scene(65, 79)
        for bad in ((good[5][0], good[5][1], 6), big, (None, good[5][1], 20), (good[5][0], None, 20)):
            pairs = list(good)
            pairs[5] = bad
            status = [np.full(80, 0xAB, np.uint8) for _ in range(S)]
            infos = (pkg.fmat.FmatInfo * S)()
            C.memset(infos, 0xAB, C.sizeof(infos))
            assert _raw_find(pkg, batch, pairs, thr, status, infos) == A.LVI_ERR_INVALID_ARG
            assert all((st == 0xAB).all() for st in status)
            assert bytes(infos) == b"\xab" * C.sizeof(infos)
            for s in range(S):
                for k, v in batch.trace(s).items():
                    np.testing.assert_array_equal(_b64(v) if k == "F" else v, _b64(before[s][k]) if k == "F" else before[s][k])
        # a null status pointer in an active slot
        status = [np.full(80, 0xAB, np.uint8) for _ in range(S)]
        status[2] = None
        assert _raw_find(pkg, batch, good, thr, status) == A.LVI_ERR_INVALID_ARG
        assert all((st == 0xAB).all() for st in status if st is not None)
        assert batch.counters() == cnt
        # the next valid call is correct
        nxt = [_scene(30 + s, 80 + s) if s % 2 else None for s in range(S)]
        _check_call(batch, singles(), nxt, thr)
        # all slots sit out: LVI_OK, nothing launched, nothing awaited
        cnt = batch.counters()
        out = batch.find([None] * S, thr)
        assert out == [None] * S
        now = batch.counters()
        assert all(now[k] == cnt[k] for k in ("hyp_launches", "walk_launches", "waits"))
        assert all(len(batch.trace(s)["subsets"]) == 0 for s in range(S))
    finally:
        batch.close()


# --------------------------------------------------------------------------------------------- 5. counters
def test_counters(pkg, hip):
    S = 8
    batch = pkg.FundamentalRansacBatch(hip, S, max_points=64)
    try:
        assert batch.counters() == dict(calls=0, hyp_launches=0, walk_launches=0, waits=0)
        want = dict(calls=0, hyp_launches=0, walk_launches=0, waits=0)
        for act in ((3,), (0, 4, 7), tuple(range(S))):
            batch.find([_scene(20 + s, 90 + s) if s in act else None for s in range(S)], 1.0)
            want = dict(calls=want["calls"] + 1, hyp_launches=want["hyp_launches"] + len(act), walk_launches=want["walk_launches"] + 1, waits=want["waits"] + 1)
            assert batch.counters() == want
        # a slot whose sample stream is empty is active (it gets its status and info) but has nothing to score
        out = batch.find([_exact_line(30) if s == 1 else _scene(20, 95) if s == 6 else None for s in range(S)], 1.0)
        assert out[1][1]["n_subsets"] == 0 and not out[1][0].any()
        want = dict(calls=want["calls"] + 1, hyp_launches=want["hyp_launches"] + 1, walk_launches=want["walk_launches"] + 1, waits=want["waits"] + 1)
        assert batch.counters() == want
    finally:
        batch.close()


# --------------------------------------------------------------------------------------------- 6. rig
def test_rig_with_the_batched_hook_equals_the_per_camera_hooks(pkg, hip):
    """the sequences, PUB patterns, cameras and parameters of test_gpu_tbatch.test_rig_equals_three_feature_trackers over 20
    frames (the scene cuts moved to frames 6, 11 and 16 so that every camera still has one): a batched rig with
    use_batched_fundamental against a batched rig with use_device_fundamental"""
    from helpers import bits
    from test_gpu_tbatch import H, W, _assert_un_equal, _rig_sequence
    import json
    import os
    ref = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_params.json")))["camera"]
    yaml_cam = {k: float(ref[k]) for k in ("xi", "k1", "k2", "p1", "p2", "gamma1", "gamma2", "u0", "v0")}
    hl = pkg.load_host()
    slots, n = 3, 20
    seqs3 = [_rig_sequence(pkg, 70 + 5 * s, n, cut) for s, cut in zip(range(slots), (6, 11, 16))]
    pub = [lambda k: True, lambda k: k % 2 == 0, lambda k: k % 3 != 1]
    cams = [dict(yaml_cam, u0=yaml_cam["u0"] * W / 1024 + 2.0 * s, v0=yaml_cam["v0"] * H / 576 - 1.5 * s) for s in range(slots)]
    tp = pkg.default_tracker_params(hip, max_width=W, max_height=H, max_features=256, max_cnt=100, min_dist=15.0)
    runs, stats = [], []
    for form in ("batched", "per_camera"):
        rig = pkg.host_api.TrackerRig(hl, tp, slots, H, W, equalize=True, cams=cams, batched=True)
        try:
            rig.use_batched_fundamental() if form == "batched" else rig.use_device_fundamental()
            rig.reset_ids()
            per_frame, per_stat = [], []
            for k in range(n):
                rig.read_images([seqs3[s][k] for s in range(slots)], [100.0 + k / 30.0 + 0.001 * s for s in range(slots)], [pub[s](k) for s in range(slots)])
                rig.update_ids()
                per_frame.append([rig.camera(s) for s in range(slots)])
                per_stat.append(rig.fundamental_stats())
            runs.append(per_frame); stats.append(per_stat)
        finally:
            rig.close()
    for k in range(n):
        for s in range(slots):
            a, b = runs[0][k][s], runs[1][k][s]
            tag = f"frame {k} camera {s}"
            np.testing.assert_array_equal(a["ids"], b["ids"], err_msg=tag)
            np.testing.assert_array_equal(a["track_cnt"], b["track_cnt"], err_msg=tag)
            np.testing.assert_array_equal(bits(a["cur_pts"]), bits(b["cur_pts"]), err_msg=tag)
            _assert_un_equal(a["cur_un_pts"], b["cur_un_pts"], tag)
            _assert_un_equal(a["pts_velocity"], b["pts_velocity"], tag)
    bat, cam = stats[0], stats[1]
    assert bat[-1]["rejectWithF_skipped"] == 0 and cam[-1]["rejectWithF_skipped"] == 0
    assert bat[-1]["rejectWithF_removed"] == cam[-1]["rejectWithF_removed"] > 0          # at least one frame removes a track
    # one batched call per frame on which a camera prepared; the per-camera hooks make one call per camera that prepared
    per_cam_calls = np.diff([0] + [c["calls"] for c in cam])
    np.testing.assert_array_equal(np.diff([0] + [b["prepared"] for b in bat]), per_cam_calls)
    np.testing.assert_array_equal(np.diff([0] + [b["calls"] for b in bat]), (per_cam_calls > 0).astype(int))
    assert (per_cam_calls >= 2).any() and bat[-1]["calls"] < cam[-1]["calls"]
    assert all(len(c["ids"]) > 50 for c in runs[0][n - 1])


def test_the_batched_hook_needs_the_batched_rig(pkg, hip):
    tp = pkg.default_tracker_params(hip, max_width=64, max_height=48, max_features=64, max_cnt=20, min_dist=5.0)
    rig = pkg.host_api.TrackerRig(pkg.load_host(), tp, 2, 48, 64, batched=False)
    try:
        with pytest.raises(pkg.LviError) as e:
            rig.use_batched_fundamental()
        assert e.value.code == pkg._abi.LVI_ERR_STATE
    finally:
        rig.close()
