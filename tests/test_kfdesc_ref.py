"""CPU tier of the keyframe describer (include/lvi_kf.h): the numpy restatement tests/kfdesc_ref.py against
known answers and literal brute forces, the BRIEF pattern fixture and its loader, and the non-vacuity of the scenes the
GPU tier (tests/test_gpu_kf.py) compares on."""
import os

import numpy as np
import pytest

import kfdesc_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
PATTERN_FILE = os.path.join(HERE, "golden", "brief_pattern.yml")


@pytest.fixture(scope="module")
def pattern(pkg):
    return pkg.config.load_brief_pattern(PATTERN_FILE)


# ------------------------------------------------------------------------------------------------------------- blur
def test_gaussian_weights_kat():
    assert R.gaussian_weights() == [7, 17, 32, 46, 52, 46, 32, 17, 7]
    assert sum(R.gaussian_weights()) == 256


@pytest.mark.parametrize("v", [0, 1, 127, 254, 255])
def test_blur_constant_image_stays_constant(v):
    assert np.all(R.blur(np.full((23, 31), v, np.uint8)) == v)


def test_blur_impulse():
    img = np.zeros((33, 41), np.uint8)
    img[16, 20] = 255
    w = R.gaussian_weights()
    want = np.zeros((33, 41), np.int64)
    for i in range(9):
        for j in range(9):
            want[16 - 4 + i, 20 - 4 + j] = (255 * w[i] * w[j] + 32768) >> 16
    assert np.array_equal(R.blur(img), want)


def test_blur_reflect101_at_all_four_borders():
    """a 16x16 ramp against a literal per-pixel loop whose index reflection is spelled out: -1 -> 1, -4 -> 4, 16 -> 14, 19 -> 11"""
    img = (np.arange(16)[:, None] * 13 + np.arange(16)[None, :] * 7).astype(np.uint8)
    w = R.gaussian_weights()

    def refl(i):
        return -i if i < 0 else (30 - i if i > 15 else i)
    assert [refl(i) for i in (-4, -1, 0, 15, 16, 19)] == [4, 1, 0, 15, 14, 11]
    want = np.zeros((16, 16), np.int64)
    for y in range(16):
        for x in range(16):
            v = 0
            for i in range(9):
                hsum = sum(w[j] * int(img[refl(y - 4 + i), refl(x - 4 + j)]) for j in range(9))
                v += w[i] * hsum
            want[y, x] = (v + 32768) >> 16
    got = R.blur(img)
    assert np.array_equal(got, want)
    # the borders are not those of a replicated or zero border
    for other in ("edge", "constant"):
        p = np.pad(img, 4, mode=other).astype(np.int64)
        hp = sum(w[j] * p[:, j:j + 16] for j in range(9))
        v = sum(w[i] * hp[i:i + 16, :] for i in range(9))
        alt = (v + 32768) >> 16
        for border in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
            assert not np.array_equal(alt[border], got[border]), other


# ------------------------------------------------------------------------------------------------------------- FAST
def _brute_force_score(img, t=R.FAST_T):
    """the largest threshold at which a pixel is still a FAST-9 corner (some arc of 9 contiguous circle pixels all darker
    than v - thr, or all brighter than v + thr), kept when the pixel is a corner at thr = t; 0 elsewhere"""
    img = np.asarray(img, np.int32)
    h, w = img.shape
    out = np.zeros((h, w), np.int32)
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            v = img[y, x]
            ring = [img[y + dy, x + dx] for dx, dy in R.CIRCLE]
            largest = -1
            for thr in range(0, 256):
                corner = False
                for a in range(16):
                    arc = [ring[(a + j) % 16] for j in range(9)]
                    if all(p < v - thr for p in arc) or all(p > v + thr for p in arc):
                        corner = True
                        break
                if not corner:
                    break                                               # a corner at thr is a corner at every smaller one
                largest = thr
            out[y, x] = largest if largest >= t else 0
    return out


@pytest.mark.parametrize("seed", [0, 1])
def test_fast_score_equals_the_brute_force(seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (32, 32)).astype(np.uint8)
    # random noise alone has few corners: plant smooth blobs so that scores of many sizes occur
    for _ in range(12):
        y, x = rng.integers(0, 28, 2)
        img[y:y + rng.integers(2, 6), x:x + rng.integers(2, 6)] = rng.integers(0, 256)
    got = R.fast_score(img).astype(np.int32)
    want = _brute_force_score(img)
    assert (want > 0).sum() > 10
    assert np.array_equal(got, want)


def test_fast_bright_square_yields_its_four_corners():
    """A two-level square ties: the corner pixel and its neighbours along both edges are all corners with the one score
    bright - dark - 1, and equal neighbours suppress each other, so nothing survives.  Shaded towards its corners (2 grey
    levels per pixel, far below the threshold) the square keeps exactly its four corner pixels."""
    flat = np.full((40, 48), 30, np.uint8)
    flat[10:26, 12:32] = 200
    sc = R.fast_score(flat)
    assert sc[10, 12] == sc[10, 13] == sc[11, 12] == 169 and len(R.fast_nms(sc)) == 0
    ys, xs = np.mgrid[0:40, 0:48]
    img = np.full((40, 48), 30, np.uint8)
    shade = (120 + 2 * (np.abs(xs - 21.5) + np.abs(ys - 17.5))).astype(np.uint8)
    img[10:26, 12:32] = shade[10:26, 12:32]
    kp = R.fast(img)
    assert sorted(map(tuple, kp.astype(int))) == sorted([(12, 10), (31, 10), (12, 25), (31, 25)])


def test_fast_finds_nothing_inside_the_border():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 52)).astype(np.uint8)
    sc = R.fast_score(img)
    assert (sc > 0).sum() > 20
    inner = np.zeros_like(sc, bool)
    inner[3:-3, 3:-3] = True
    assert np.all(sc[~inner] == 0)
    kp = R.fast(img)
    assert len(kp) and kp[:, 0].min() >= 3 and kp[:, 0].max() < 52 - 3 and kp[:, 1].min() >= 3 and kp[:, 1].max() < 40 - 3


def test_nms_equal_neighbours_suppress_both_and_order_is_row_major():
    sc = np.zeros((12, 12), np.uint8)
    sc[4, 4] = sc[4, 5] = 50                                            # equal neighbours: neither is strictly greater
    sc[8, 8] = 60; sc[8, 9] = 59                                        # the larger survives
    sc[6, 2] = 40; sc[3, 9] = 30; sc[6, 10] = 25
    kp = R.fast_nms(sc)
    assert kp.dtype == np.float32
    assert [tuple(p) for p in kp.astype(int)] == [(9, 3), (2, 6), (10, 6), (8, 8)]


# ------------------------------------------------------------------------------------------------------------- BRIEF
def _pattern_with(first):
    pat = [np.zeros(256, np.int32) for _ in range(4)]
    for a, v in zip(pat, first):
        a[0] = v
    return pat


def test_brief_truncates_towards_zero():
    """(0.6, 0.6) with offset -1: the sum -0.4 truncates to pixel 0, in the image (a floor would give -1 and bit 0)"""
    img = np.full((16, 16), 100, np.uint8)
    img[0, 0] = 10
    pat = _pattern_with((-1, -1, 3, 3))                                 # blur[0][0] = 10 < blur[3][3] = 100
    d = R.brief(img, [(0.6, 0.6)], pat)
    assert d[0, 0] & np.uint64(1) == 1
    assert R.brief(img, [(0.6, 0.6)], _pattern_with((3, 3, -1, -1)))[0, 0] & np.uint64(1) == 0     # the comparison is strict and directed
    # -1.0 exactly is outside: (0.0, 0.0) with offset -1
    assert R.brief(img, [(0.0, 0.0)], pat)[0, 0] & np.uint64(1) == 0


def test_brief_pair_leaving_the_image_gives_bit_zero():
    img = np.zeros((16, 20), np.uint8)
    img[:, 10:] = 200
    inside = _pattern_with((-5, 0, 5, 0))
    assert R.brief(img, [(8.0, 8.0)], inside)[0, 0] & np.uint64(1) == 1
    for pt in [(2.0, 8.0), (19.5, 8.0)]:                                # x1 < 0; x2 = 24.5 >= 20
        assert R.brief(img, [pt], inside)[0, 0] & np.uint64(1) == 0
    vert = _pattern_with((0, -9, 5, 0))
    assert R.brief(img, [(8.0, 8.0)], vert)[0, 0] & np.uint64(1) == 0    # y1 = -1
    assert R.brief(img, [(8.0, 8.5)], vert)[0, 0] & np.uint64(1) == 1    # y1 = -0.5 -> row 0
    assert R.brief(img, [(np.nan, 8.0)], inside)[0, 0] == 0


@pytest.mark.parametrize("i", [0, 1, 63, 64, 127, 128, 200, 255])
def test_brief_word_and_bit_layout(i):
    img = np.zeros((16, 20), np.uint8)
    img[:, 10:] = 200
    pat = [np.zeros(256, np.int32) for _ in range(4)]
    pat[0][i], pat[2][i] = -5, 5                                        # only pair i compares dark < bright
    d = R.brief(img, [(8.0, 8.0)], pat)[0]
    want = np.zeros(4, np.uint64)
    want[i >> 6] = np.uint64(1) << np.uint64(i & 63)
    assert np.array_equal(d, want)


# ------------------------------------------------------------------------------------------------------------- match
def _flip(desc, bits):
    d = np.array(desc, np.uint64).copy()
    for b in bits:
        d[b >> 6] ^= np.uint64(1) << np.uint64(b & 63)
    return d


def test_match_tie_goes_to_the_lowest_index():
    rng = np.random.default_rng(5)
    q = rng.integers(0, 2 ** 63, 4).astype(np.uint64)
    far = _flip(q, range(100))
    old = np.stack([far, _flip(q, [3, 70, 200]), _flip(q, [5, 90, 255]), _flip(q, [1, 2, 3])])
    st, ix, ds = R.match(q[None], old)
    assert (st[0], ix[0], ds[0]) == (1, 1, 3)


def test_match_accepts_79_and_rejects_80():
    q = np.zeros(4, np.uint64)
    st, ix, ds = R.match(np.stack([q, q]), np.stack([_flip(q, range(79))]))
    assert list(st) == [1, 1] and list(ds) == [79, 79]
    st, ix, ds = R.match(q[None], np.stack([_flip(q, range(80))]))
    assert (st[0], ix[0], ds[0]) == (0, 0, 80)                          # a best was found, but it is not below 80


def test_match_distance_128_never_becomes_a_best():
    q = np.zeros(4, np.uint64)
    old = np.stack([_flip(q, range(128)), _flip(q, range(200)), _flip(q, range(256))])
    st, ix, ds = R.match(q[None], old)
    assert (st[0], ix[0], ds[0]) == (0, -1, 128)
    st, ix, ds = R.match(q[None], np.concatenate([old, _flip(q, range(127))[None]]))
    assert (st[0], ix[0], ds[0]) == (0, 3, 127)


def test_match_empty_old_set():
    st, ix, ds = R.match(np.zeros((5, 4), np.uint64), np.zeros((0, 4), np.uint64))
    assert list(st) == [0] * 5 and list(ix) == [-1] * 5 and list(ds) == [128] * 5
    st, ix, ds = R.match(np.zeros((0, 4), np.uint64), np.zeros((3, 4), np.uint64))
    assert len(st) == len(ix) == len(ds) == 0


def test_hamming_is_the_bit_count():
    rng = np.random.default_rng(9)
    a = rng.integers(0, 2 ** 63, (3, 4)).astype(np.uint64)
    b = rng.integers(0, 2 ** 63, (5, 4)).astype(np.uint64)
    want = [[sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(ra, rb)) for rb in b] for ra in a]
    assert np.array_equal(R.hamming(a, b), want)


# ------------------------------------------------------------------------------------------------------------- fixture and scenes
def test_brief_pattern_fixture_and_loader(pkg, pattern, tmp_path):
    assert len(pattern) == 4 and all(len(p) == 256 for p in pattern)
    flat = np.array(pattern)
    assert flat.min() >= -24 and flat.max() <= 24 and flat.min() < 0 < flat.max()
    assert (pattern[0][:5], pattern[0][-1]) == ([0, 4, 11, -4, 24], pattern[0][255])
    bad = tmp_path / "short.yml"
    bad.write_text("%YAML:1.0\nx1: [1, 2]\ny1: [1, 2]\nx2: [1, 2]\ny2: [1, 2]\n")
    with pytest.raises(ValueError):
        pkg.config.load_brief_pattern(str(bad))
    far = tmp_path / "far.yml"
    body = "".join(f"{k}:\n" + "".join(f"  - {25 if (k == 'y2' and i == 7) else 1}\n" for i in range(256)) for k in ("x1", "y1", "x2", "y2"))
    far.write_text("%YAML:1.0\n" + body)
    with pytest.raises(ValueError):
        pkg.config.load_brief_pattern(str(far))


def test_scenes_are_not_vacuous(pkg):
    S = pkg.synth
    assert len(R.fast(S.make_texture(320, 240, 4242))) > 100
    assert len(R.fast(S.make_texture(157, 93, 7))) > 50


def test_match_scene_is_not_vacuous(pkg, pattern):
    """the scene pair of the GPU tier: the reference alone accepts more than MIN_LOOP_NUM matches, and they are the right ones"""
    S = pkg.synth
    img0, img1, win, sel = R.scene_pair(S)
    assert len(win) == 150 and np.any(win != np.round(win))             # sub-pixel window points
    d0 = R.describe(img0, np.zeros((0, 2)), pattern)
    d1 = R.describe(img1, win, pattern)
    st, ix, ds = R.match(d1["win_desc"], d0["kp_desc"])
    assert st.sum() > R.MIN_LOOP_NUM
    assert (ix[st == 1] == sel[st == 1]).mean() > 0.9
