"""TEST INFRASTRUCTURE — exact reference of the VoxelGrid centroids (csrc/lvi_voxel.hpp).

model_centroids evaluates the contract of the HIP realisations exactly, per voxel and per coordinate:

    cell  = floor(f32(v * f32(1 / leaf)))                      PCL's key expression (the voxel a point belongs to)
    k     = 37 - ex,  2 * leaf = f * 2^ex with f in [0.5, 1)   (frexp)
    q_i   = RNE(2^k * RN64(v_i - cell * leaf))                 an integer; RN64 is exact unless |v_i| < 2^-28 leaf in cell -1
    value = RNE_f32(cell * leaf + sum(q_i) / (cnt * 2^k))      rounded once

and for the intensity q_i = RNE(2^ki * I_i), value = RNE_f32(sum(q_i) / (cnt * 2^ki)) with
ki = 37 - max(ex(max |I| over the segment), 8), or ki = 29 on the incremental map.

exact_centroids gives the correctly rounded true mean of the raw f32 values of every voxel.  Both work on Python / numpy
integers only; numpy f32 arithmetic appears in the key expression alone, which defines membership.  Never imported by the
product package."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
INT32_MAX = 2 ** 31 - 1


def f32_parts(a):
    """v = m * 2^e exactly: int64 arrays m (|m| < 2^24, 0 for zeros) and e"""
    u = np.ascontiguousarray(a, F32).reshape(-1).view(np.uint32).astype(np.int64)
    eb = (u >> 23) & 0xFF
    assert np.all(eb < 255), "inf / nan"
    frac = u & 0x7FFFFF
    m = np.where(eb > 0, frac | (1 << 23), frac)
    e = np.where(eb > 0, eb - 150, -149)
    return np.where((u >> 31) == 1, -m, m), e


def leaf_parts(leaf):
    m, e = f32_parts(np.array([leaf], F32))
    return int(m[0]), int(e[0])


def fx_k(leaf):
    return 37 - math.frexp(float(F32(2) * F32(leaf)))[1]


def fx_ki(intensity=None, incremental=False):
    """intensity scale of a segment: from its largest |intensity|, never coarser than 2^-29; 29 on the incremental map"""
    if incremental:
        return 29
    a = np.abs(np.asarray(intensity, F32))
    return 37 - max(math.frexp(float(a.max()) if a.size else 0.0)[1], 8)


def round_sig(n, d, bits):
    """n / d (Python ints, d > 0) rounded to `bits` significant bits, ties to even: (m, e) with value m * 2^e"""
    if n == 0:
        return 0, 0
    s = -1 if n < 0 else 1
    n = abs(n)
    e = n.bit_length() - d.bit_length() - bits
    while True:
        num, den = (n << -e, d) if e < 0 else (n, d << e)
        q, r = divmod(num, den)
        if q >= 1 << bits:
            e += 1
        elif q < 1 << (bits - 1):
            e -= 1
        else:
            break
    if 2 * r > den or (2 * r == den and q & 1):
        q += 1
    return s * q, e


def f32_of(n, d=1):
    """RNE_f32(n / d) from Python ints: one rounding (float(Fraction) then f32 would round twice); subnormal results are
    rounded on the 2^-149 grid"""
    n, d = int(n), int(d)
    m, e = round_sig(n, d, 24)
    if m != 0 and e + 23 < -126:
        m, e = rne_div(n << 149, d), -149
    return F32(math.ldexp(m, e))


def rne_div(n, d):
    """RNE(n / d), Python ints, d > 0"""
    q, r = divmod(n, d)
    if 2 * r > d or (2 * r == d and q & 1):
        q += 1
    return q


def rne_shift(m, s):
    """RNE(m * 2^s) of int64 arrays (|m| < 2^40)"""
    m = np.asarray(m, np.int64)
    s = np.asarray(s, np.int64)
    out = np.zeros_like(m)
    p = s >= 0
    out[p] = np.left_shift(m[p], s[p])
    n = ~p
    a, sh = np.abs(m[n]), np.minimum(-s[n], 62)
    q = np.right_shift(a, sh)
    rem = a - np.left_shift(q, sh)
    half = np.left_shift(np.int64(1), sh - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    out[n] = np.where(m[n] < 0, -q, q)
    return out


def pcl_cells(xyz, leaf):
    """absolute voxel coordinates floor(f32(v * inv)), inv = f32(1 / leaf) (setLeafSize, applyFilter)"""
    inv = F32(1) / F32(leaf)
    c = np.floor(np.asarray(xyz, F32) * inv)
    assert np.all(np.abs(c) < 2 ** 26), "cell out of the contract's range (|cell| < 2^26, DESIGN §2)"
    return c.astype(np.int64)


def pcl_overflow(xyz, leaf):
    """PCL's "leaf size too small" rule: output = input"""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    if len(xyz) == 0:
        return False
    inv = F32(1) / F32(leaf)
    d = [int(np.trunc(F32(xyz[:, j].max() - xyz[:, j].min()) * inv)) + 1 for j in range(3)]
    return d[0] * d[1] * d[2] > INT32_MAX


def q_xyz(v, cell, leaf, k):
    """q_i = RNE(2^k * RN64(v_i - cell_i * leaf)) for one coordinate: int64 array"""
    mv, ev = f32_parts(v)
    cell = np.asarray(cell, np.int64)
    ml, el = leaf_parts(leaf)
    assert el + k == 12                                      # leaf * 2^k = ml * 2^12: cell * leaf is a multiple of 2^-k
    C = cell * (ml << 12)
    s = ev + k
    q = np.zeros(len(mv), np.int64)
    fast = (s >= 0) & (s <= 38)                              # v * 2^k an integer: the offset is exact, no rounding at all
    q[fast] = np.left_shift(mv[fast], s[fast]) - C[fast]
    zero = ~fast & (cell == 0) & (s < 0)                     # offset = v itself, exact in binary64
    q[zero] = rne_shift(mv[zero], s[zero])
    for i in np.nonzero(~(fast | zero))[0]:                  # v - cell * leaf rounded to binary64 first (cell -1, |v| tiny)
        x = Fraction(int(mv[i])) * Fraction(2) ** int(ev[i]) - int(cell[i]) * Fraction(ml) * Fraction(2) ** el
        m, e = round_sig(x.numerator, x.denominator, 53)
        q[i] = m << (e + k) if e + k >= 0 else rne_div(m, 1 << -(e + k))
    return q


def q_int(intensity, ki):
    m, e = f32_parts(intensity)
    return rne_shift(m, e + ki)


def _voxels(pts, leaf):
    """PCL's voxels in output order (ascending linear idx = (z, y, x) lexicographic): order, run starts, cells, counts"""
    p = np.ascontiguousarray(pts)
    p = p.view(F32).reshape(-1, 4) if p.dtype.names else p.astype(F32, copy=False).reshape(-1, 4)
    cells = pcl_cells(p[:, :3], leaf)
    order = np.lexsort((cells[:, 0], cells[:, 1], cells[:, 2]))
    cs = cells[order]
    head = np.ones(len(cs), bool)
    head[1:] = np.any(cs[1:] != cs[:-1], axis=1)
    starts = np.nonzero(head)[0]
    counts = np.diff(np.append(starts, len(cs)))
    return p, order, starts, cs[starts], counts


def model_centroids(pts, leaf, ki=None):
    """the HIP realisations' centroids of one VoxelGrid segment: dict(cells (nvox, 3) int64, counts, pts (nvox, 4) f32,
    k, ki).  ki defaults to the segment's own scale (fx_ki); the incremental map passes 29."""
    p, order, starts, cells, counts = _voxels(pts, leaf)
    assert not pcl_overflow(p[:, :3], leaf), "PCL's overflow rule fires: output = input"
    k = fx_k(leaf)
    if ki is None:
        ki = fx_ki(p[:, 3])
    ml, _ = leaf_parts(leaf)
    out = np.zeros((len(starts), 4), F32)
    if len(p) == 0:
        return dict(cells=cells, counts=counts, pts=out, k=k, ki=ki)
    ps = p[order]
    cpt = pcl_cells(ps[:, :3], leaf)
    sums = [np.add.reduceat(q_xyz(ps[:, d], cpt[:, d], leaf, k), starts) for d in range(3)]
    sums.append(np.add.reduceat(q_int(ps[:, 3], ki), starts))
    den_x, den_i = 1 << k, 1 << ki
    for v in range(len(starts)):
        n = int(counts[v])
        for d in range(3):
            C = int(cells[v, d]) * (ml << 12)
            out[v, d] = f32_of(C * n + int(sums[d][v]), n * den_x)
        out[v, 3] = f32_of(int(sums[3][v]), n * den_i)
    return dict(cells=cells, counts=counts, pts=out, k=k, ki=ki)


def exact_centroids(pts, leaf):
    """the correctly rounded true mean of the raw f32 values of every voxel: (nvox, 4) f32 in model_centroids' order"""
    p, order, starts, cells, counts = _voxels(pts, leaf)
    out = np.zeros((len(starts), 4), F32)
    if len(p) == 0:
        return out
    vid = np.repeat(np.arange(len(starts)), counts)
    ps = p[order]
    for d in range(4):
        m, e = f32_parts(ps[:, d])
        o = np.lexsort((e, vid))                                # vid ascending already; exponent groups inside each voxel
        vo, eo, mo = vid[o], e[o], m[o]
        head = np.ones(len(o), bool)
        head[1:] = (vo[1:] != vo[:-1]) | (eo[1:] != eo[:-1])
        gs = np.nonzero(head)[0]
        gsum = np.add.reduceat(mo, gs)                          # |m| < 2^24, <= 2^25 points: exact in int64
        gv, ge = vo[gs], eo[gs]
        bounds = np.searchsorted(gv, np.arange(len(starts) + 1))
        for v in range(len(starts)):
            a, b = bounds[v], bounds[v + 1]
            emin = int(ge[a])
            tot = sum(int(gsum[j]) << (int(ge[j]) - emin) for j in range(a, b))
            n = int(counts[v])
            out[v, d] = f32_of(tot << emin, n) if emin >= 0 else f32_of(tot, n << -emin)
    return out


def half_ulp(a):
    a = np.abs(np.asarray(a, F32)).astype(np.float64)
    return 0.5 * (np.nextafter(np.asarray(a, F32), F32(np.inf)).astype(np.float64) - a)


def model_bound(leaf, k, ki):
    """|model - true mean| per component, before the final rounding: half a step of the fixed-point grid (xyz: plus the
    binary64 rounding of the offset in the band where it is inexact)"""
    lf = float(F32(leaf))
    return np.array([2.0 ** -(k + 1) + 2.0 ** -52 * lf] * 3 + [2.0 ** -(ki + 1)])


def within_bound(model, exact, leaf, k, ki):
    """|model - exact| <= model_bound + half an ulp of each, component-wise: bool (nvox, 4)"""
    m, e = np.asarray(model, F32), np.asarray(exact, F32)
    diff = np.abs(m.astype(np.float64) - e.astype(np.float64))
    return diff <= model_bound(leaf, k, ki)[None, :] + half_ulp(m) + half_ulp(e)
