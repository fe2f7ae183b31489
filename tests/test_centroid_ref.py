"""CPU tier: the exact centroid reference (centroid_ref.py) against hand-computed voxels, and the oracle's centroid switch
(lvo_set_centroid_mode) against the reference."""
import ctypes
import math
from fractions import Fraction

import numpy as np

import centroid_ref as R
from helpers import xyzi

F32 = np.float32


def _cloud(xyz, inten=None):
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    p = np.zeros((len(xyz), 4), F32)
    p[:, :3] = xyz
    p[:, 3] = 0 if inten is None else inten
    return p


def _nextf(v, n=1):
    v = F32(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, F32(np.inf if n > 0 else -np.inf))
    return v


def test_round_once_to_f32():
    one = Fraction(1)
    assert R.f32_of(3, 2) == F32(1.5)
    # exact midpoints go to the even neighbour
    assert R.f32_of(2 ** 24 + 1, 2 ** 24) == F32(1.0)                      # 1 + 2^-24: between 1 (even) and 1 + 2^-23
    assert R.f32_of(2 ** 24 + 3, 2 ** 24) == F32(1 + 2 ** -22)             # 1 + 3 * 2^-24: between odd and even
    assert R.f32_of(-(2 ** 24 + 1), 2 ** 24) == F32(-1.0)
    # just above a midpoint by less than half a binary64 ulp: float(Fraction) lands on the midpoint, then f32 rounds to even
    x = one + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)
    assert F32(float(x)) == F32(1.0)                                        # the double rounding the reference must avoid
    assert R.f32_of(x.numerator, x.denominator) == F32(1 + 2 ** -23)
    assert R.f32_of(0, 7) == F32(0)
    assert R.f32_of(1, 2 ** 149) == np.nextafter(F32(0), F32(1)) and R.f32_of(3, 2 ** 150) == 2 * np.nextafter(F32(0), F32(1))
    assert R.f32_of(1, 2 ** 150) == F32(0)                                  # half the smallest subnormal: tie to even (zero)
    assert math.ldexp(*R.round_sig(7, 2, 2)) == 4.0 and math.ldexp(*R.round_sig(5, 2, 2)) == 2.0   # 3.5 -> 4, 2.5 -> 2
    assert R.rne_div(5, 2) == 2 and R.rne_div(7, 2) == 4 and R.rne_div(-5, 2) == -2
    np.testing.assert_array_equal(R.rne_shift(np.array([5, 7, -5, -7, 6, 3]), np.array([-1, -1, -1, -1, -2, 2])), [2, 4, -2, -4, 2, 12])


def test_scales_follow_the_device_setup():
    assert R.fx_k(0.4) == 37 - 0 and R.fx_k(0.5) == 36 and R.fx_k(5.0) == 37 - 4 and R.fx_k(0.02) == 37 + 4
    assert R.fx_ki([0.0, 255.99]) == 29 and R.fx_ki([-300.0]) == 28 and R.fx_ki([1e5]) == 20 and R.fx_ki([]) == 29
    assert R.fx_ki(None, incremental=True) == 29


def test_hand_computed_voxels():
    leaf = 0.5
    pts = _cloud([[0.25, 0.5, -0.25], [0.125, 0.75, -0.125], [-0.25, 1.25, 7.0], [-0.125, 1.0, 7.125], [-0.5, 1.0, 7.25]],
                 [1.0, 2.0, 10.0, 20.0, 31.0])
    m = R.model_centroids(pts, leaf)
    np.testing.assert_array_equal(m["cells"], [[0, 1, -1], [-1, 2, 14]])   # ordered by (z, y, x)
    np.testing.assert_array_equal(m["counts"], [2, 3])
    np.testing.assert_array_equal(m["pts"], F32([[0.1875, 0.625, -0.1875, 1.5], [-0.875 / 3, 3.25 / 3, 21.375 / 3, 61.0 / 3]]))
    np.testing.assert_array_equal(R.exact_centroids(pts, leaf), m["pts"])


def test_model_ties_to_even():
    # two points one ulp apart at 1.0 / 1 + 2^-23: their mean is an exact f32 midpoint
    for a, b, want in ((1.0, _nextf(1.0), F32(1.0)), (_nextf(1.0), _nextf(1.0, 2), _nextf(1.0, 2)),
                       (-1.0, _nextf(-1.0, -1), F32(-1.0))):
        pts = _cloud([[a, 0.5, 0.5], [b, 0.5, 0.5]])
        m = R.model_centroids(pts, 4.0)
        assert m["pts"][0, 0] == want and R.exact_centroids(pts, 4.0)[0, 0] == want


def test_one_point_voxels_away_from_zero_are_the_point():
    rng = np.random.default_rng(3)
    for leaf in (0.4, 0.2, 0.1, 0.25, 0.02, 5.0):
        xyz = rng.uniform(-2000, 2000, (3000, 3)).astype(F32)
        xyz[:1000] = rng.uniform(-3, 3, (1000, 3))
        xyz[np.abs(xyz) < 1e-2] = F32(0.5)
        pts = _cloud(xyz, rng.uniform(-5, 255.99, 3000))
        for i in range(0, 3000, 500):                     # PCL's overflow rule keeps the cloud small; one point per call
            one = pts[i:i + 1]
            m = R.model_centroids(one, leaf)
            np.testing.assert_array_equal(m["pts"].view(np.uint32), one.view(np.uint32), err_msg=f"leaf {leaf}")
            np.testing.assert_array_equal(R.exact_centroids(one, leaf).view(np.uint32), one.view(np.uint32))


def test_near_zero_band_is_within_the_stated_bound():
    """below ~2^(24-k) a coordinate has bits finer than the 2^-k grid: the model is not the point, but within the bound"""
    leaf = 0.4
    k = R.fx_k(leaf)
    for x, ulps_min in ((3e-5, 1), (-1e-9, 1000), (-3e-5, 1), (1e-9, 1000)):
        one = _cloud([[x, 0.1, 0.1]])
        m = R.model_centroids(one, leaf)
        got, want = m["pts"][0, 0], one[0, 0]
        ulps = abs(int(np.array(got, F32).view(np.int32)) - int(np.array(want, F32).view(np.int32)))
        assert ulps >= ulps_min, (x, got)
        assert abs(float(got) - float(want)) <= 2.0 ** -(k + 1) + 2.0 ** -52 * 0.4 + float(R.half_ulp(got)), (x, got)
        assert R.within_bound(m["pts"], R.exact_centroids(one, leaf), leaf, k, m["ki"]).all()
    # intensity: one large value coarsens the whole segment's grid to 2^-20
    pts = _cloud([[1.1, 1.1, 1.1], [5.1, 1.1, 1.1]], [1e5, 1e-3])
    m = R.model_centroids(pts, 0.4)
    assert m["ki"] == 20 and m["pts"][0, 3] == F32(1e5)
    assert m["pts"][1, 3] == F32(2 ** -20 * round(float(F32(1e-3)) * 2 ** 20)) != F32(1e-3)


def test_binary64_band_of_the_offset():
    """cell -1 and |v| < 2^-28 leaf: v - cell*leaf is rounded to binary64 before the grid; the model follows the device"""
    leaf = 0.5
    k = R.fx_k(leaf)
    v = -F32(2.0 ** -40 + 2.0 ** -63)
    q = R.q_xyz(np.array([v], F32), np.array([-1]), leaf, k)[0]
    assert R.pcl_cells(np.array([v]), leaf)[0] == -1
    x64 = float(Fraction(1, 2) + Fraction(float(v)))                     # one binary64 rounding, as the device forms it
    assert q == R.rne_div(int(Fraction(x64) * 2 ** k * 2 ** 80), 2 ** 80)


def test_model_and_exact_agree_within_the_bound_on_dense_voxels():
    rng = np.random.default_rng(11)
    for leaf in (0.4, 0.02, 5.0):
        n = 20000
        c = rng.integers(-3, 3, (n, 3))
        xyz = ((c + rng.uniform(0, 1, (n, 3))) * leaf).astype(F32)
        xyz[:50] = rng.uniform(-1e-6, 1e-6, (50, 3))
        pts = _cloud(xyz, rng.uniform(-3, 255.99, n))
        m = R.model_centroids(pts, leaf)
        e = R.exact_centroids(pts, leaf)
        assert len(m["pts"]) <= 216 and m["counts"].sum() == n
        assert R.within_bound(m["pts"], e, leaf, m["k"], m["ki"]).all()


def _switch(oracle):
    d = oracle.dll
    d.lvo_set_centroid_mode.argtypes = [ctypes.c_int]
    d.lvo_set_centroid_mode.restype = None
    d.lvo_get_centroid_mode.restype = ctypes.c_int
    return d


def _switch_cloud():
    rng = np.random.default_rng(5)
    parts = [rng.uniform(-30, 30, (6000, 3)),
             np.repeat(rng.uniform(-5, 5, (8, 3)), 700, axis=0) + rng.uniform(-0.05, 0.05, (5600, 3)),
             rng.uniform(-1e-4, 1e-4, (300, 3)),
             np.array([[0.4, -0.4, 0.0], [-1e-9, 3e-5, -3e-5], [2.0, -2.0, 0.8]])]
    xyz = np.concatenate(parts).astype(F32)
    return _cloud(xyz, rng.uniform(-2, 255.99, len(xyz)))


def test_oracle_centroid_switch(pkg, oracle):
    """mode 1 is centroid_ref's model bit for bit; mode 0 (PCL's f32 sums) is unchanged by a round trip"""
    A = pkg._abi
    d = _switch(oracle)
    assert d.lvo_get_centroid_mode() == 0
    o = pkg.LidarHotpath(oracle, N_SCAN=4, Horizon_SCAN=1000, max_raw_points=4096, max_map_points=20000)
    pts = _switch_cloud()
    before = {leaf: o.voxel_downsample(pts, leaf) for leaf in (0.4, 0.2, 0.05)}
    try:
        d.lvo_set_centroid_mode(1)
        assert d.lvo_get_centroid_mode() == 1
        for leaf in (0.4, 0.2, 0.05):
            got = xyzi(o.voxel_downsample(pts, leaf))
            m = R.model_centroids(pts, leaf)
            np.testing.assert_array_equal(o.debug_get(A.DBG_VOXEL_COUNTS, np.int32), m["counts"])
            np.testing.assert_array_equal(got.view(np.uint32), m["pts"].view(np.uint32), err_msg=f"leaf {leaf}")
            assert (got != xyzi(before[leaf])).any()                       # the switch does change something
    finally:
        d.lvo_set_centroid_mode(0)
    assert d.lvo_get_centroid_mode() == 0
    for leaf in (0.4, 0.2, 0.05):
        np.testing.assert_array_equal(xyzi(o.voxel_downsample(pts, leaf)).view(np.uint32), xyzi(before[leaf]).view(np.uint32))
    o.close()
