"""Exact / float64 references of the visual front end, written from SURVEY App. A.6 (calcOpticalFlowPyrLK) and A.7
(goodFeaturesToTrack) alone: numpy and Python integers, no line shared with oracle/ or the HIP kernels.

What is exact here and what is not (DESIGN "Tracker references"):
  * pyramid, Scharr derivatives, the bilinear fixed-point patches and the five sums A11 A12 A22 b1 b2 are integers;
  * `lk_step_exact` takes its start on the 1/64-pixel grid, where the four weights are integers before rounding: the only
    inexact operation of a step is the 2x2 solve, done here in rationals and rounded once to float64;
  * `lk_track_ref` carries float32 positions and takes the weights by the float32 rule of A.6 (each operation one IEEE
    rounding, so an implementation that follows A.6 gets the same integers), the sums exactly and the solve in float64;
  * `mineig_ref` forms the Sobel products and their 3x3 box sums as integers and the eigenvalue in float64;
  * `gftt_select` is exact from a given float32 map.
One point the appendix leaves implicit and OpenCV's tracker has: after the last iteration of level 0 the window is tested
against the exits once more before `err` is taken (a point that stepped out with its last step gets status 0)."""
from fractions import Fraction

import numpy as np

F32 = np.float32
W_BITS = 14
FLT_EPSILON = float(np.finfo(np.float32).eps)       # 1.1920929e-7
INF = float("inf")


# ----------------------------------------------------------------------------- pyramid
def reflect_idx(i, n):
    """BORDER_REFLECT_101 to any depth: ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ..."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def pyrdown(img):
    """[1 4 6 4 1]x[1 4 6 4 1], REFLECT_101, (sum + 128) >> 8, size (w+1)/2 x (h+1)/2"""
    k = np.array([1, 4, 6, 4, 1], np.int64)
    h, w = img.shape
    p = img.astype(np.int64)[np.ix_(reflect_idx(np.arange(-2, h + 2), h), reflect_idx(np.arange(-2, w + 2), w))]
    tmp = sum(k[i] * p[:, i:i + w] for i in range(5))
    full = sum(k[j] * tmp[j:j + h, :] for j in range(5))
    return ((full[::2, ::2] + 128) >> 8).astype(np.uint8)


def build_pyramid(img, win, max_level):
    """buildOpticalFlowPyramid: level L is built; if the NEXT size ((w+1)/2, (h+1)/2) is <= win in either direction, L is the top"""
    pyr = [np.ascontiguousarray(img, np.uint8)]
    h, w = pyr[0].shape
    for level in range(max_level + 1):
        if level:
            pyr.append(pyrdown(pyr[-1]))
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win or h <= win:
            break
    return pyr


def scharr(img):
    """[-1 0 1] x [3 10 3] unnormalised, REFLECT_101 neighbours at in-image pixels → (dx, dy) int64"""
    h, w = img.shape
    p = img.astype(np.int64)[np.ix_(reflect_idx(np.arange(-1, h + 1), h), reflect_idx(np.arange(-1, w + 1), w))]
    sm_y = 3 * p[:-2, :] + 10 * p[1:-1, :] + 3 * p[2:, :]        # smoothed down the column, (h, w + 2)
    sm_x = 3 * p[:, :-2] + 10 * p[:, 1:-1] + 3 * p[:, 2:]        # smoothed along the row, (h + 2, w)
    return sm_y[:, 2:] - sm_y[:, :-2], sm_x[2:, :] - sm_x[:-2, :]


# ----------------------------------------------------------------------------- patches
def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def weights_f32(fx, fy):
    """a, b = the float32 fractional parts; cvRound is half-to-even; iw11 is the remainder"""
    a, b = F32(fx), F32(fy)
    one, s = F32(1), F32(1 << W_BITS)
    w00 = int(np.rint((one - a) * (one - b) * s))
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10


def patch(src, ix, iy, win, wts, shift, zero_outside=False):
    """DESCALE(sum w * src, shift) over the win x win window whose corner is (ix, iy).  src int64 (h, w); outside the level
    the source is REFLECT_101 (images) or zero (derivatives)"""
    h, w = src.shape
    ys, xs = np.arange(iy, iy + win + 1), np.arange(ix, ix + win + 1)
    if zero_outside:
        t = src[np.ix_(np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1))]
        t = t * (((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :])
    else:
        t = src[np.ix_(reflect_idx(ys, h), reflect_idx(xs, w))]
    w00, w01, w10, w11 = wts
    return descale(w00 * t[:-1, :-1] + w01 * t[:-1, 1:] + w10 * t[1:, :-1] + w11 * t[1:, 1:], shift)


def _isum(a):
    return int(a.sum(dtype=np.int64))         # |terms| < 2^31 and at most 441 of them: no overflow


def _gates(s11, s12, s22, win):
    """A11 A12 A22 (x 2^-20), D and minEig in float64 from the exact sums"""
    sc = 2.0 ** -20
    A11, A12, A22 = s11 * sc, s12 * sc, s22 * sc
    D = float(Fraction(s11 * s22 - s12 * s12, 1 << 40))
    # the stable form of A11 + A22 - sqrt((A11 - A22)^2 + 4 A12^2): 2 D / (trace + root) loses nothing to cancellation
    root = np.sqrt((A11 - A22) ** 2 + 4.0 * A12 * A12)
    tr = A11 + A22
    min_eig = (2.0 * D / (tr + root) if tr + root > 0 else 0.0) / (win * win)
    return A11, A12, A22, D, min_eig


def _gate_margin(A11, A22, D, min_eig, thr, win):
    """relative distance of the two gates from their boundaries, taken against the magnitude of what a float32 evaluation rounds:
    minEig is a difference of terms of size (A11 + A22) / (2 win^2), D of terms of size A11 A22"""
    m1 = abs(min_eig - thr) / max(thr, (A11 + A22) / (2.0 * win * win), 1e-300)
    m2 = abs(D - FLT_EPSILON) / max(FLT_EPSILON, A11 * A22)
    return min(m1, m2)


def _exit(ix, iy, win, w, h):
    return ix < -win or ix >= w or iy < -win or iy >= h


def _solve(s11, s12, s22, b1, b2):
    """delta = ((A12 b2 - A22 b1) / D, (A12 b1 - A11 b2) / D): the scales 2^-20 cancel; exact rationals, one rounding"""
    det = s11 * s22 - s12 * s12
    return float(Fraction(s12 * b2 - s22 * b1, det)), float(Fraction(s12 * b1 - s11 * b2, det))


def lk_step_exact(I, J, pt64, win, min_eig=1e-4):
    """one Lucas-Kanade step at level 0 from a start given in 1/64 pixel (integers pt64 = 64 * (x, y)).
    Returns a dict: status (after the gates and exits of a one-iteration call), sums (A11, A12, A22, b1, b2 as integers),
    delta (float64), err (sum|J - I| / (32 win^2) at the START, i.e. what a zero-iteration call reports), err_sum (the integer),
    minEig, D, sx / sy (conditioning of the two components), margin (of the gates), gate (True if tracked past them)"""
    qx, qy = int(pt64[0]), int(pt64[1])
    assert (qx, qy) == (pt64[0], pt64[1]), "the start is not on the 1/64 grid"
    half = (win - 1) // 2
    px, py = qx - 64 * half, qy - 64 * half
    ix, iy = px // 64, py // 64
    fa, fb = px - 64 * ix, py - 64 * iy                               # 64 * a, 64 * b
    # (1 - a)(1 - b) 2^14 = 4 (64 - fa)(64 - fb): integers before any rounding
    exact = (4 * (64 - fa) * (64 - fb), 4 * fa * (64 - fb), 4 * (64 - fa) * fb, 4 * fa * fb)
    for v, (ca, cb) in zip(exact[:3], (((64 - fa), (64 - fb)), (fa, (64 - fb)), ((64 - fa), fb))):
        assert float(ca / 64.0 * (cb / 64.0) * (1 << W_BITS)).is_integer() and int(ca / 64.0 * (cb / 64.0) * (1 << W_BITS)) == v
    assert exact == weights_f32(fa / 64.0, fb / 64.0) and sum(exact) == 1 << W_BITS
    h, w = I.shape
    out = dict(status=1, sums=None, delta=(0.0, 0.0), err=0.0, err_sum=0, minEig=0.0, D=0.0, sx=0.0, sy=0.0, margin=INF, gate=False,
               exit_prev=False)
    if _exit(ix, iy, win, w, h):
        out.update(status=0, exit_prev=True)
        return out
    I64, J64 = I.astype(np.int64), J.astype(np.int64)
    dx, dy = scharr(I)
    Iw = patch(I64, ix, iy, win, exact, W_BITS - 5)
    Ix = patch(dx, ix, iy, win, exact, W_BITS, zero_outside=True)
    Iy = patch(dy, ix, iy, win, exact, W_BITS, zero_outside=True)
    s11, s12, s22 = _isum(Ix * Ix), _isum(Ix * Iy), _isum(Iy * Iy)
    A11, A12, A22, D, me = _gates(s11, s12, s22, win)
    out.update(minEig=me, D=D, margin=_gate_margin(A11, A22, D, me, float(F32(min_eig)), win))
    diff = patch(J64, ix, iy, win, exact, W_BITS - 5) - Iw             # no initial flow: the target window starts where the source's is
    b1, b2 = _isum(diff * Ix), _isum(diff * Iy)
    out["sums"] = (s11, s12, s22, b1, b2)
    if me < float(F32(min_eig)) or D < FLT_EPSILON:
        out["status"] = 0
        return out
    out["gate"] = True
    out["err_sum"] = _isum(np.abs(diff))
    out["err"] = out["err_sum"] / (32.0 * win * win)
    out["delta"] = _solve(s11, s12, s22, b1, b2)
    # after its step a one-iteration call tests the moved window against the exits once more (status1); the start's own tests
    # are exact on the 1/64 grid and carry no margin
    nx, ny = px / 64.0 + out["delta"][0], py / 64.0 + out["delta"][1]
    out["status1"] = 0 if _exit(int(np.floor(nx)), int(np.floor(ny)), win, w, h) else 1
    out["margin1"] = min(out["margin"], _exit_margin(nx, ny, win, w, h))
    sc = 2.0 ** -20
    k = A11 * A22 / D
    out["sx"] = k * (abs(A12 * b2 * sc) + abs(A22 * b1 * sc)) / D
    out["sy"] = k * (abs(A12 * b1 * sc) + abs(A11 * b2 * sc)) / D
    return out


# ----------------------------------------------------------------------------- the pyramidal tracker
END_EXIT_PREV, END_GATE, END_EXIT, END_EPS, END_OSC, END_ITERS = "exit_prev", "gate", "exit", "eps", "osc", "iters"


def _rel(v, bound):
    return abs(v - bound) / bound if bound > 0 else (INF if v != bound else 0.0)


def lk_track_ref(pyrI, pyrJ, pts, win, max_level, max_iters, eps, min_eig):
    """calcOpticalFlowPyrLK without initial flow over prebuilt pyramids (lists, level 0 first).  Positions are float32 and every
    position operation (pt * 2^-L, 2 * next, -halfWin, +delta, +halfWin, x - floor(x), the weight products) is one IEEE
    float32 operation; sums are exact, gates and the solve float64.  Returns a dict of per-point arrays / lists:
    status, xy (float32), err (float64), iters[p][L], ended[p][L], travel (greatest whole-pixel displacement of the target window's
    corner from where it stood at the start of its level, either axis), margin"""
    top = min(max_level, len(pyrI) - 1, len(pyrJ) - 1)
    max_iters = min(max(int(max_iters), 0), 100)
    eps = min(max(float(eps), 0.0), 10.0)
    eps2 = eps * eps
    thr = float(F32(min_eig))
    half = F32((win - 1) * 0.5)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    I64 = [a.astype(np.int64) for a in pyrI]
    J64 = [a.astype(np.int64) for a in pyrJ]
    dI = [scharr(a) if l <= top else None for l, a in enumerate(pyrI)]
    res = dict(status=np.ones(n, np.uint8), xy=np.zeros((n, 2), np.float32), err=np.zeros(n), iters=[], ended=[],
               travel=np.zeros(n, np.int64), margin=np.full(n, INF))
    for p in range(n):
        st, errv, margin, travel = 1, 0.0, INF, 0
        iters, ended = {}, {}
        outx = outy = F32(0)
        for level in range(top, -1, -1):
            h, w = pyrI[level].shape
            hj, wj = pyrJ[level].shape
            sc = F32(1.0 / (1 << level))
            prevx, prevy = pts[p, 0] * sc, pts[p, 1] * sc
            if level == top:
                nextx, nexty = prevx, prevy
            else:
                nextx, nexty = outx * F32(2), outy * F32(2)
            outx, outy = nextx, nexty
            prevx, prevy = prevx - half, prevy - half
            ipx, ipy = int(np.floor(prevx)), int(np.floor(prevy))
            iters[level] = 0
            margin = min(margin, _exit_margin(float(prevx), float(prevy), win, w, h))
            if _exit(ipx, ipy, win, w, h):
                if level == 0:
                    st, errv = 0, 0.0
                ended[level] = END_EXIT_PREV
                continue
            wts = weights_f32(prevx - F32(ipx), prevy - F32(ipy))
            Iw = patch(I64[level], ipx, ipy, win, wts, W_BITS - 5)
            Ix = patch(dI[level][0], ipx, ipy, win, wts, W_BITS, zero_outside=True)
            Iy = patch(dI[level][1], ipx, ipy, win, wts, W_BITS, zero_outside=True)
            s11, s12, s22 = _isum(Ix * Ix), _isum(Ix * Iy), _isum(Iy * Iy)
            A11, A12, A22, D, me = _gates(s11, s12, s22, win)
            margin = min(margin, _gate_margin(A11, A22, D, me, thr, win))
            if me < thr or D < FLT_EPSILON:
                if level == 0:
                    st = 0
                ended[level] = END_GATE
                continue
            nextx, nexty = nextx - half, nexty - half
            pdx = pdy = 0.0
            ended[level] = END_ITERS
            ox0 = oy0 = None
            for j in range(max_iters):
                inx, iny = int(np.floor(nextx)), int(np.floor(nexty))
                margin = min(margin, _exit_margin(float(nextx), float(nexty), win, wj, hj))
                if _exit(inx, iny, win, wj, hj):
                    if level == 0:
                        st = 0
                    ended[level] = END_EXIT
                    break
                if ox0 is None:
                    ox0, oy0 = inx, iny
                travel = max(travel, abs(inx - ox0), abs(iny - oy0))
                wts = weights_f32(nextx - F32(inx), nexty - F32(iny))
                diff = patch(J64[level], inx, iny, win, wts, W_BITS - 5) - Iw
                b1, b2 = _isum(diff * Ix), _isum(diff * Iy)
                dx, dy = _solve(s11, s12, s22, b1, b2)
                nextx, nexty = F32(float(nextx) + dx), F32(float(nexty) + dy)
                outx, outy = nextx + half, nexty + half
                iters[level] = j + 1
                d2 = dx * dx + dy * dy
                margin = min(margin, _rel(d2, eps2))
                if d2 <= eps2:
                    ended[level] = END_EPS
                    break
                if j > 0:
                    ax, ay = abs(dx + pdx), abs(dy + pdy)
                    mx, my = _rel(ax, 0.01), _rel(ay, 0.01)
                    if ax < 0.01 and ay < 0.01:
                        margin = min(margin, mx, my)
                        outx, outy = outx - F32(F32(dx) * F32(0.5)), outy - F32(F32(dy) * F32(0.5))
                        ended[level] = END_OSC
                        break
                    margin = min(margin, max(mx if ax >= 0.01 else 0.0, my if ay >= 0.01 else 0.0))
                pdx, pdy = dx, dy
            if st and level == 0:
                nx, ny = outx - half, outy - half
                inx, iny = int(np.floor(nx)), int(np.floor(ny))
                margin = min(margin, _exit_margin(float(nx), float(ny), win, wj, hj))
                if _exit(inx, iny, win, wj, hj):
                    st = 0
                    continue
                wts = weights_f32(nx - F32(inx), ny - F32(iny))
                diff = patch(J64[0], inx, iny, win, wts, W_BITS - 5) - Iw
                errv = _isum(np.abs(diff)) / (32.0 * win * win)
        res["status"][p] = st
        res["xy"][p] = (outx, outy)
        res["err"][p] = errv
        res["iters"].append(iters)
        res["ended"].append(ended)
        res["travel"][p] = travel
        res["margin"][p] = margin
    res["settled"] = np.array([END_ITERS not in e.values() for e in res["ended"]], bool)
    return res


def _exit_margin(x, y, win, w, h):
    """distance of a window corner from the four exit boundaries (floor(x) < -win ⇔ x < -win; floor(x) >= w ⇔ x >= w), relative to
    the boundary's magnitude"""
    return min(abs(x + win) / win, abs(x - w) / w, abs(y + win) / win, abs(y - h) / h)


def ulp32(x):
    """spacing of float32 at |x| (float64 in, float64 out)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ----------------------------------------------------------------------------- cornerMinEigenVal / goodFeaturesToTrack
MINEIG_SCALE = 3060                       # 1 / (2^(3-1) * 3 * 255)


def _box3(a):
    h, w = a.shape
    p = a[np.ix_(reflect_idx(np.arange(-1, h + 1), h), reflect_idx(np.arange(-1, w + 1), w))]
    return sum(p[j:j + h, i:i + w] for j in range(3) for i in range(3))


def mineig_ref(img):
    """cornerMinEigenVal(blockSize 3, Sobel 3): returns (eig, a + c) in float64; Sobel, products and box sums are exact integers"""
    h, w = img.shape
    p = img.astype(np.int64)[np.ix_(reflect_idx(np.arange(-1, h + 1), h), reflect_idx(np.arange(-1, w + 1), w))]
    sm_y = p[:-2, :] + 2 * p[1:-1, :] + p[2:, :]
    sm_x = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
    Dx, Dy = sm_y[:, 2:] - sm_y[:, :-2], sm_x[2:, :] - sm_x[:-2, :]
    sxx, sxy, syy = _box3(Dx * Dx), _box3(Dx * Dy), _box3(Dy * Dy)
    k = float(MINEIG_SCALE) ** 2
    a, b, c = sxx / (2.0 * k), sxy / k, syy / (2.0 * k)
    return (a + c) - np.sqrt((a - c) ** 2 + b * b), a + c


def mineig_unit(apc):
    """the unit of the min-eigenvalue tolerance: float32 rounding of a value of size a + c, plus the absolute error 2^-24 / 3 of a
    separable float32 Sobel's smoothed-row difference entering (a + c) through 2 * Dy * dDy (DESIGN)"""
    return 2.0 ** -24 * (apc + 2.0 * np.sqrt(2.0 * apc))


def gftt_candidates(eig_f32, mask, quality):
    """(thr, candidate mask): interior pixels that survive THRESH_TOZERO, are non-zero, equal their 3x3 dilation and have mask != 0"""
    e = np.asarray(eig_f32, np.float32)
    h, w = e.shape
    m = np.ones((h, w), bool) if mask is None else (np.asarray(mask) != 0)
    mx = float(e[m].max()) if m.any() else 0.0
    thr = F32(mx * float(quality))
    t = np.where(e > thr, e, F32(0))
    cand = np.zeros((h, w), bool)
    if h >= 3 and w >= 3:
        dil = t[1:-1, 1:-1].copy()
        for j in range(3):
            for i in range(3):
                dil = np.maximum(dil, t[j:j + h - 2, i:i + w - 2])
        c = t[1:-1, 1:-1]
        cand[1:-1, 1:-1] = (c != 0) & (c == dil) & m[1:-1, 1:-1]
    return thr, cand


def gftt_select(eig_f32, mask, quality, min_dist, max_corners):
    """goodFeaturesToTrack's selection from a given float32 min-eigenvalue map → (corners (k, 2) float32 as (x, y), candidate count)"""
    e = np.asarray(eig_f32, np.float32)
    h, w = e.shape
    _, cand = gftt_candidates(e, mask, quality)
    addr = np.flatnonzero(cand.ravel())
    vals = e.ravel()[addr]
    order = np.lexsort((-addr, -vals.astype(np.float64)))          # descending value, higher address first among equal values
    addr = addr[order]
    out = []
    md2 = float(min_dist) * float(min_dist)
    if min_dist >= 1:
        ax, ay = np.zeros(len(addr)), np.zeros(len(addr))
        k = 0
        for a in addr:
            y, x = divmod(int(a), w)
            if k == 0 or not (((ax[:k] - x) ** 2 + (ay[:k] - y) ** 2) < md2).any():
                ax[k], ay[k] = x, y
                k += 1
                out.append((x, y))
                if max_corners > 0 and k == max_corners:
                    break
    else:
        for a in addr:
            y, x = divmod(int(a), w)
            out.append((x, y))
            if max_corners > 0 and len(out) == max_corners:
                break
    return np.array(out, np.float32).reshape(-1, 2), len(addr)
