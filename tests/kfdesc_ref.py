"""numpy restatement of the pose_graph keyframe front end (pose_graph/src/keyframe.cpp:14-131, 266-271): the parity
target of include/lvi_kf.h.  It restates OpenCV 4.5.x and DVision in integer arithmetic; it is not OpenCV.

    blur     cv::GaussianBlur(u8, Size(9, 9), 2, 2), the bit-exact fixed-point path: 8.8 weights, BORDER_REFLECT_101
    fast     cv::FAST(image, keypoints, 20, true): FAST-9/16 on the unblurred image, 3x3 non-max suppression, row-major
    brief    DVision::BRIEF::compute on the blurred image: 256 pairs, f32 sum truncated towards zero, 4 x u64 per point
    match    KeyFrame::searchInAera over every window descriptor: bestDist 128, strict <, accepted below 80
"""
import numpy as np

KSIZE, SIGMA = 9, 2.0
FAST_T = 20
MATCH_START, MATCH_ACCEPT = 128, 80
MIN_LOOP_NUM = 25
# (dx, dy) of the 16 circle pixels, in OpenCV's order
CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2),
          (-1, 3))


# ------------------------------------------------------------------------------------------------------------- blur
def gaussian_weights(ksize=KSIZE, sigma=SIGMA):
    """8.8 fixed-point weights of OpenCV's bit-exact Gaussian kernel: exp(-x^2 / (2 sigma^2)) normalised, rounded from the
    left end towards the centre with the rounding error carried into the next tap, the centre = 256 - 2 * sum."""
    r = ksize // 2
    x = np.arange(-r, r + 1, dtype=np.float64)
    k = np.exp(-x * x / (2.0 * sigma * sigma))
    k /= k.sum()
    w = [0] * ksize
    err = 0.0
    for i in range(r):
        v = k[i] * 256.0 + err
        q = int(np.floor(v + 0.5))
        err = v - q
        w[i] = w[ksize - 1 - i] = q
    w[r] = 256 - 2 * sum(w[:r])
    return w


def reflect101(i, n):
    i = np.asarray(i)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def blur(img):
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    wt = gaussian_weights()
    r = len(wt) // 2
    cols = reflect101(np.arange(-r, w + r), w)
    rows = reflect101(np.arange(-r, h + r), h)
    src = img.astype(np.uint32)[:, cols]                              # [h, w + 2r]
    hp = np.zeros((h, w), np.uint32)
    for k, wk in enumerate(wt):
        hp += wk * src[:, k:k + w]
    assert hp.max() <= 0xFFFF                                         # the u16 intermediate cannot overflow
    hp = hp[rows, :]                                                  # [h + 2r, w]
    v = np.zeros((h, w), np.uint32)
    for k, wk in enumerate(wt):
        v += wk * hp[k:k + h, :]
    return ((v + 32768) >> 16).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- FAST
def circle_diffs(img):
    """d[k] = v - p_k for the pixels 3 <= x < w-3, 3 <= y < h-3: int32 [16, h-6, w-6]"""
    a = np.asarray(img, np.uint8).astype(np.int32)
    h, w = a.shape
    v = a[3:h - 3, 3:w - 3]
    return np.stack([v - a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRCLE])


def fast_score(img, t=FAST_T):
    """the score map (u8): best - 1 where best > t, else 0, with best = max over the 16 arcs of 9 contiguous circle pixels
    of min(d) and of min(-d).  Equals OpenCV's cornerScore<16> (the largest threshold at which the pixel is still a corner)."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    d = circle_diffs(img)
    best = np.full(d.shape[1:], -256, np.int32)
    for a in range(16):
        arc = [(a + j) % 16 for j in range(9)]
        best = np.maximum(best, d[arc].min(axis=0))
        best = np.maximum(best, (-d[arc]).min(axis=0))
    out = np.zeros((h, w), np.uint8)
    out[3:h - 3, 3:w - 3] = np.where(best > t, best - 1, 0).astype(np.uint8)
    return out


def fast_nms(score):
    """keypoints (x, y) float32 [n, 2], row-major: score > 0 and strictly greater than all 8 neighbours"""
    s = np.asarray(score, np.uint8).astype(np.int32)
    h, w = s.shape
    p = np.zeros((h + 2, w + 2), np.int32)
    p[1:-1, 1:-1] = s
    keep = s > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= s > p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    ys, xs = np.nonzero(keep)                                         # np.nonzero is row-major
    return np.stack([xs, ys], axis=1).astype(np.float32)


def fast(img, t=FAST_T):
    return fast_nms(fast_score(img, t))


# ------------------------------------------------------------------------------------------------------------- BRIEF
def brief(blurred, pts, pattern):
    """pts [n, 2] float32 (x, y); pattern = (x1, y1, x2, y2), 256 ints each -> uint64 [n, 4]"""
    b = np.asarray(blurred, np.uint8)
    h, w = b.shape
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    x1, y1, x2, y2 = [np.asarray(a, np.int32).astype(np.float32) for a in pattern]
    out = np.zeros((len(pts), 4), np.uint64)
    for n, (px, py) in enumerate(pts):
        sums = [np.float32(px) + x1, np.float32(py) + y1, np.float32(px) + x2, np.float32(py) + y2]      # f32 additions
        lim = [w, h, w, h]
        inb = np.ones(256, bool)
        for s, m in zip(sums, lim):
            inb &= (s > np.float32(-1.0)) & (s < np.float32(m))       # NaN compares false: out of the image
        X1, Y1, X2, Y2 = [np.where(inb, s, np.float32(0)).astype(np.int32) for s in sums]               # the cast truncates towards zero
        bits = inb & (b[Y1, X1] < b[Y2, X2])
        out[n] = np.packbits(bits.reshape(4, 64), axis=1, bitorder="little").view("<u8").reshape(4)
    return out


# ------------------------------------------------------------------------------------------------------------- match
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def hamming(a, b):
    """a [n, 4], b [m, 4] uint64 -> int32 [n, m]"""
    a = np.ascontiguousarray(a, np.uint64).reshape(-1, 4)
    b = np.ascontiguousarray(b, np.uint64).reshape(-1, 4)
    out = np.zeros((len(a), len(b)), np.int32)
    for i in range(len(a)):                                            # row by row: [m, 32] bytes at a time
        out[i] = _POP8[(a[i][None, :] ^ b).view(np.uint8)].sum(axis=1, dtype=np.int32)
    return out


def match(window_desc, old_desc):
    """(status u8 [n], index i32 [n], dist i32 [n]): the lowest-index old descriptor with the smallest distance below 128
    (index -1, dist 128 when there is none); status = found and dist < 80"""
    window_desc = np.ascontiguousarray(window_desc, np.uint64).reshape(-1, 4)
    n = len(window_desc)
    index = np.full(n, -1, np.int32)
    dist = np.full(n, MATCH_START, np.int32)
    if len(old_desc):
        d = hamming(window_desc, old_desc)
        j = d.argmin(axis=1)                                           # the first minimum: strict <
        dm = d[np.arange(n), j]
        found = dm < MATCH_START
        index[found] = j[found]
        dist[found] = dm[found]
    status = ((index >= 0) & (dist < MATCH_ACCEPT)).astype(np.uint8)
    return status, index, dist


# ------------------------------------------------------------------------------------------------------------- keyframe
def describe(img, window_xy, pattern, max_keypoints=None):
    """the KeyFrame constructor's image work: dict(blur, score, keypoints, n_found, kp_desc, win_desc)"""
    bl = blur(img)
    sc = fast_score(img)
    kp = fast_nms(sc)
    n_found = len(kp)
    if max_keypoints is not None:
        kp = kp[:max_keypoints]
    win = np.ascontiguousarray(window_xy, np.float32).reshape(-1, 2)
    return dict(blur=bl, score=sc, keypoints=kp, n_found=n_found, kp_desc=brief(bl, kp, pattern), win_desc=brief(bl, win, pattern))


def find_connection_front(cur, old):
    """findConnection up to PnPRANSAC.  cur: dict(win_desc, point_2d_uv, point_2d_norm, point_3d, point_id); old:
    dict(kp_desc, keypoints, keypoints_norm) -> (passes the > MIN_LOOP_NUM gate, dict of the six compacted vectors)"""
    status, index, _ = match(cur["win_desc"], old["kp_desc"])
    n = len(status)
    old_xy = np.zeros((n, 2), np.float32)
    old_norm = np.zeros((n, 2), np.float32)
    ok = status == 1
    old_xy[ok] = np.asarray(old["keypoints"], np.float32)[index[ok]]
    old_norm[ok] = np.asarray(old["keypoints_norm"], np.float32)[index[ok]]
    out = dict(matched_2d_cur=np.asarray(cur["point_2d_uv"], np.float32)[ok], matched_2d_old=old_xy[ok],
               matched_2d_cur_norm=np.asarray(cur["point_2d_norm"], np.float32)[ok], matched_2d_old_norm=old_norm[ok],
               matched_3d=np.asarray(cur["point_3d"], np.float32)[ok], matched_id=np.asarray(cur["point_id"], np.float64)[ok])
    return int(ok.sum()) > MIN_LOOP_NUM, out


def scene_pair(S, w=320, h=240, seed=4242, hseed=100, max_px=6.0, n_window=150):
    """the match scene of the tests: frame 0 and its homography warp; old keypoints = FAST on frame 0, window points = an
    evenly spaced n_window subset of them mapped into frame 1 (sub-pixel).  S = the package's synth module."""
    img0 = S.make_texture(w, h, seed)
    Hm = S.small_motion_homography(w, h, hseed, max_px)
    img1 = S.warp_homography(img0, Hm)
    kp0 = fast(img0)
    sel = np.linspace(0, len(kp0) - 1, min(n_window, len(kp0))).astype(int)
    win = S.apply_homography(Hm, kp0[sel]).astype(np.float32)
    inside = (win[:, 0] >= 0) & (win[:, 0] <= w - 1) & (win[:, 1] >= 0) & (win[:, 1] <= h - 1)
    return img0, img1, win[inside], sel[inside]
