"""GPU tier of the keyframe describer (include/lvi_kf.h) against the numpy restatement tests/kfdesc_ref.py.
Everything but the normalised keypoints is integer arithmetic, so every comparison is exact: no tolerance, no allowed
share of mismatches.  The normalised keypoints are compared bit for bit with the oracle's lvi_undistort_points."""
import ctypes as C
import os

import numpy as np
import pytest

import kfdesc_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W0, H0 = 320, 240


@pytest.fixture(scope="module")
def pattern(pkg):
    return pkg.config.load_brief_pattern(os.path.join(HERE, "golden", "brief_pattern.yml"))


@pytest.fixture(scope="module")
def cam(pkg):
    return pkg.config.load_camera_yaml(os.path.join(HERE, "golden", "params_camera.yaml"))[1]


@pytest.fixture(scope="module")
def kd(pkg, hip, pattern):
    h = pkg.KeyframeDescriber(hip, pattern, max_width=W0, max_height=H0, max_keypoints=5000, max_window=150, max_keyframes=6)
    yield h
    h.close()


def _window_points(w, h, n=150, seed=11):
    """n sub-pixel points: the corners' neighbourhood (0.6, 0.6) first, then points within 24 pixels of each border,
    the rest anywhere in the image"""
    rng = np.random.default_rng(seed)
    pts = [(0.6, 0.6), (w - 1.0, h - 1.0), (0.0, 0.0), (w - 1.4, 0.3), (0.25, h - 1.25)]
    for k in range(10):
        pts += [(rng.uniform(0, 24), rng.uniform(0, h - 1)), (rng.uniform(w - 25, w - 1), rng.uniform(0, h - 1)),
                (rng.uniform(0, w - 1), rng.uniform(0, 24)), (rng.uniform(0, w - 1), rng.uniform(h - 25, h - 1))]
    while len(pts) < n:
        pts.append((rng.uniform(0, w - 1), rng.uniform(0, h - 1)))
    return np.array(pts[:n], np.float32)


def _image(pkg, w, h):
    if (w, h) == (320, 240):
        return pkg.synth.make_texture(320, 240, 4242)
    if (w, h) == (157, 93):
        return pkg.synth.make_texture(157, 93, 7)
    return np.random.default_rng(16).integers(0, 256, (h, w)).astype(np.uint8)     # 16x16: the smallest image, noise


@pytest.fixture(scope="module")
def refs(pkg, pattern):
    """the restatement's answers, computed once per size: {(w, h): (img, window points, describe dict)}"""
    out = {}
    for w, h in ((320, 240), (157, 93), (16, 16)):
        img = _image(pkg, w, h)
        win = _window_points(w, h)
        out[(w, h)] = (img, win, R.describe(img, win, pattern))
    return out


SIZES = [(320, 240), (157, 93), (16, 16)]


@pytest.mark.parametrize("size", SIZES)
def test_describe_is_exact(kd, refs, cam, size):
    """blur, score map, keypoints (count, coordinates, order) and all four words of every descriptor"""
    img, win, ref = refs[size]
    info = kd.describe(0, img, win, cam)
    bl, sc = kd.debug_maps()
    assert np.array_equal(bl, ref["blur"])
    assert np.array_equal(sc, ref["score"])
    assert info["n_keypoints_found"] == info["n_keypoints_stored"] == len(ref["keypoints"]) and not info["truncated"]
    if size != (16, 16):
        assert len(ref["keypoints"]) > 50
    got = kd.get(0)
    assert np.array_equal(got["keypoints"], ref["keypoints"])
    assert np.array_equal(got["kp_desc"], ref["kp_desc"])
    assert np.array_equal(got["window_xy"].view(np.uint32), win.view(np.uint32))
    assert np.array_equal(got["win_desc"], ref["win_desc"])
    assert np.any(ref["win_desc"][0] != 0)                              # the (0.6, 0.6) point has pairs inside the image


def test_describe_with_a_row_stride(kd, refs):
    img, win, ref = refs[(320, 240)]
    wide = np.full((240, 352), 255, np.uint8)
    wide[:, :320] = img
    view = wide[:, :320]
    assert view.strides == (352, 1)
    kd.describe(1, view, win)
    bl, sc = kd.debug_maps()
    got = kd.get(1)
    assert np.array_equal(bl, ref["blur"]) and np.array_equal(sc, ref["score"])
    assert np.array_equal(got["keypoints"], ref["keypoints"]) and np.array_equal(got["kp_desc"], ref["kp_desc"])
    assert np.array_equal(got["win_desc"], ref["win_desc"])
    assert np.all(got["keypoints_norm"] == 0)                           # no camera model: zeros


@pytest.mark.parametrize("n_window", [0, 1, 150])
def test_window_counts(kd, refs, n_window):
    img, win, ref = refs[(157, 93)]
    info = kd.describe(2, img, win[:n_window])
    got = kd.get(2)
    assert info["n_window"] == n_window and got["win_desc"].shape == (n_window, 4)
    assert np.array_equal(got["win_desc"], ref["win_desc"][:n_window])
    assert np.array_equal(got["kp_desc"], ref["kp_desc"])


def test_truncation(pkg, hip, pattern, refs):
    img, win, ref = refs[(320, 240)]
    small = pkg.KeyframeDescriber(hip, pattern, max_width=W0, max_height=H0, max_keypoints=64, max_window=150, max_keyframes=1)
    try:
        assert len(ref["keypoints"]) > 64
        info = small.describe(0, img, win)
        assert info["truncated"] and info["n_keypoints_found"] == len(ref["keypoints"]) and info["n_keypoints_stored"] == 64
        got = small.get(0)
        assert np.array_equal(got["keypoints"], ref["keypoints"][:64])
        assert np.array_equal(got["kp_desc"], ref["kp_desc"][:64])
        assert np.array_equal(got["win_desc"], ref["win_desc"])
    finally:
        small.close()


def test_normalised_keypoints_equal_the_oracle(pkg, oracle, kd, refs, cam):
    img, win, ref = refs[(320, 240)]
    kd.describe(0, img, win, cam)
    got = kd.get(0)["keypoints_norm"]
    t = pkg.TrackerHotpath(oracle, max_width=W0, max_height=H0)
    try:
        want = t.undistort_points(cam, ref["keypoints"])
    finally:
        t.close()
    assert len(want) > 100 and np.all(np.isfinite(want)) and np.any(want != 0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------- match
@pytest.fixture(scope="module")
def scene(pkg, pattern):
    img0, img1, win, sel = R.scene_pair(pkg.synth)
    d0 = R.describe(img0, np.zeros((0, 2)), pattern)
    d1 = R.describe(img1, win, pattern)
    return img0, img1, win, d0, d1


def test_match_on_the_scene_pair(kd, scene):
    img0, img1, win, d0, d1 = scene
    kd.describe(0, img0)
    kd.describe(1, img1, win)
    st, ix, ds = kd.match(1, 0)
    rs, ri, rd = R.match(d1["win_desc"], d0["kp_desc"])
    assert rs.sum() > R.MIN_LOOP_NUM
    assert np.array_equal(st, rs) and np.array_equal(ix, ri) and np.array_equal(ds, rd)


def _flip(desc, bits):
    d = desc.copy()
    for b in bits:
        d[b >> 6] ^= np.uint64(1) << np.uint64(b & 63)
    return d


def _random_sets(m, n=150, seed=0):
    """m old descriptors and n queries: queries planted at exactly 79 and 80 bits from an old descriptor, old descriptors
    duplicated (ties), queries equal to an old descriptor, and plain random ones"""
    rng = np.random.default_rng(1000 + m + seed)
    old = rng.integers(0, 2 ** 64, (m, 4), dtype=np.uint64)
    if m >= 2:
        for k in range(max(1, m // 8)):                                 # duplicates at a higher index: ties
            a, b = sorted(rng.integers(0, m, 2))
            old[b] = old[a]
    q = rng.integers(0, 2 ** 64, (n, 4), dtype=np.uint64)
    if m:
        for i in range(0, n - 10):
            j = int(rng.integers(0, m))
            k = (79, 80, 0, 40, 127, 128)[i % 6]
            q[i] = _flip(old[j], rng.choice(256, k, replace=False))
    return old, q


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 1000, 5000])
def test_match_on_random_sets(kd, m):
    old, q = _random_sets(m)
    kd.put(3, kp_desc=old)
    kd.put(4, win_desc=q)
    st, ix, ds = kd.match(4, 3)
    rs, ri, rd = R.match(q, old)
    if m == 0:
        assert not st.any() and np.all(ix == -1) and np.all(ds == 128)
    else:
        assert 79 in rd[rs == 1] and 80 in rd[rs == 0]
    if m >= 63:
        lowest_of_a_tie = [(old[:i] == old[i]).all(axis=1).any() for i in ri[ri >= 0]]
        assert not any(lowest_of_a_tie)                                 # never the later copy of a duplicate ...
        assert any((old[i + 1:] == old[i]).all(axis=1).any() for i in ri[ri >= 0])      # ... and ties did occur
    assert np.array_equal(st, rs) and np.array_equal(ix, ri) and np.array_equal(ds, rd)


def test_store(pkg, kd, scene, refs):
    """slots are independent: release and re-describe the middle one, copy a slot through get/put, match again"""
    img0, img1, win, d0, d1 = scene
    other = refs[(157, 93)][0]
    kd.describe(0, img0)
    kd.describe(1, other, refs[(157, 93)][1])
    kd.describe(2, img1, win)
    want = R.match(d1["win_desc"], d0["kp_desc"])
    first = kd.match(2, 0)
    kd.release(1)
    with pytest.raises(pkg.LviError):
        kd.get(1)
    kd.describe(1, img0)                                                # the old keyframe again, in the freed slot
    again = kd.match(2, 1)
    copy = kd.get(0)
    kd.put(5, **{k: copy[k] for k in ("keypoints", "keypoints_norm", "kp_desc", "window_xy", "win_desc")})
    back = kd.get(5)
    through_put = kd.match(2, 5)
    for got in (first, again, through_put):
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    for k in copy:
        assert np.array_equal(back[k], copy[k]), k
    kd.release(5)


def test_host_mirror(pkg, hip, pattern, scene, cam):
    """host_api.KeyFrameMatcher (lvi_host::KeyFrameDescriber) against the restatement of findConnection's front half"""
    img0, img1, win, d0, d1 = scene
    hl = pkg.load_host()
    km = pkg.host_api.KeyFrameMatcher(hl, pattern, max_width=W0, max_height=H0, max_keypoints=5000, max_window=150, max_keyframes=3)
    t = pkg.TrackerHotpath(hip, max_width=W0, max_height=H0)
    try:
        rng = np.random.default_rng(77)
        n = len(win)
        p3 = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
        ids = np.arange(n, dtype=np.float64) * 3 + 1000
        nm = t.undistort_points(cam, win)
        kp_norm = t.undistort_points(cam, d0["keypoints"])
        i0 = km.add(0, img0, np.zeros((0, 3)), np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0), cam)
        assert i0["n_keypoints_stored"] == len(d0["keypoints"])
        old = dict(kp_desc=d0["kp_desc"], keypoints=d0["keypoints"], keypoints_norm=kp_norm)
        for slot, k in ((1, n), (2, 20)):                               # 20 window points cannot pass the > 25 gate
            km.add(slot, img1, p3[:k], win[:k], nm[:k], ids[:k], cam)
            ok, got = km.findConnectionFront(slot, 0)
            cur = dict(win_desc=d1["win_desc"][:k], point_2d_uv=win[:k], point_2d_norm=nm[:k], point_3d=p3[:k], point_id=ids[:k])
            rok, want = R.find_connection_front(cur, old)
            assert ok == rok == (k == n)
            assert len(want["matched_id"]) == (R.match(cur["win_desc"], old["kp_desc"])[0]).sum() > 0
            for key, v in want.items():
                assert got[key].shape == v.shape and np.array_equal(got[key].view(np.uint8), v.view(np.uint8)), key
    finally:
        t.close()
        km.close()


# ------------------------------------------------------------------------------------------------------------- invalid arguments
def test_invalid_arguments_write_nothing(pkg, hip, kd, refs, pattern):
    img, win, ref = refs[(157, 93)]
    kd.describe(0, img, win)
    before = kd.get(0)
    INV = pkg._abi.LVI_ERR_INVALID_ARG
    bad = [(np.zeros((H0 + 1, W0), np.uint8), win),                      # over capacity
           (np.zeros((H0, W0 + 1), np.uint8), win),
           (np.zeros((15, 15), np.uint8), win),                         # below 16x16
           (np.zeros((15, 64), np.uint8), win), (np.zeros((64, 15), np.uint8), win),
           (img, np.zeros((151, 2), np.float32))]                       # n_window > max_window
    for im, wn in bad:
        with pytest.raises(pkg.LviError) as e:
            kd.describe(0, im, wn)
        assert e.value.code == INV
    with pytest.raises(pkg.LviError) as e:
        kd.describe(6, img, win)                                        # no such slot
    assert e.value.code == INV
    after = kd.get(0)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    # match against a released and against a never-used slot: the raw call, sentinel-filled outputs
    kd.release(4)
    dll = hip.dll
    for cur, old in ((0, 4), (4, 0), (0, 6), (-1, 0)):
        st = np.full(150, 7, np.uint8); ix = np.full(150, 7, np.int32); ds = np.full(150, 7, np.int32)
        code = dll.lvi_kf_match(kd._h, cur, old, st.ctypes.data_as(C.c_void_p), ix.ctypes.data_as(C.c_void_p), ds.ctypes.data_as(C.c_void_p))
        assert code == INV
        assert np.all(st == 7) and np.all(ix == 7) and np.all(ds == 7)
    fresh = pkg.KeyframeDescriber(hip, pattern, max_width=32, max_height=32, max_keypoints=8, max_window=4, max_keyframes=2)
    try:
        st = np.full(4, 7, np.uint8)
        assert dll.lvi_kf_match(fresh._h, 0, 1, st.ctypes.data_as(C.c_void_p), None, None) == INV and np.all(st == 7)     # empty slots
    finally:
        fresh.close()


def test_abi_and_signature_table(pkg, hip):
    import re
    root = os.path.dirname(HERE)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "lvi_kf.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(lvi_kf_[a-z0-9_]+)\s*\(", txt))) == sorted(pkg.kf.KF_SIGNATURES)
    pkg.kf.bind(hip)
    assert hip.dll.lvi_kf_abi_version() == 1 and hip.dll.lvi_abi_version() == 6
