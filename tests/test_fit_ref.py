"""CPU tier: the float64 reference of the corner line fit and the surf plane fit (tests/fit_ref.py) against closed forms, then the
ORACLE against the reference on the hand-built neighbourhoods of tests/fit_scenes.py and on make_small_scene ("boxes").  This
is where the caps and the yardstick of tests/test_gpu_fit.py are established: how many features are undecidable, that the
oracle takes every decidable decision as float64 does, and how far its coefficients are from float64 per class."""
import numpy as np
import pytest

import fit_ref as R
import fit_scenes as S
from helpers import make_small_scene, small_params


# ----------------------------------------------------------------------------- the reference against closed forms
def _rot(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q


def test_cross_eigenvalue_ratio_is_the_squared_axis_ratio():
    """five points on a cross with half-axes a and b in any plane: eigenvalues 2a^2/5, 2b^2/5, 0"""
    rng = np.random.default_rng(1)
    for r in (1.0, 1.5, 2.999, 3.001, 7.0, 30.0):
        u, w, _ = _rot(rng).T
        c, b = rng.uniform(-50, 50, 3), 0.12
        a = b * np.sqrt(r)
        nb = np.array([c, c + a * u, c - a * u, c + b * w, c - b * w])
        res = R.corner(nb[None], (c + [0.02, 0.03, 0.05])[None])
        np.testing.assert_allclose(res["eigenvalues"][0], [2 * a * a / 5, 2 * b * b / 5, 0.0], atol=1e-12)
        assert abs(res["ratio"][0] - r) <= 1e-9 * r
        assert bool(res["flag"][0]) == (r > 3.0)
        if r > 1.0:
            assert abs(abs(res["direction"][0] @ u) - 1.0) <= 1e-9


def test_line_coefficients_closed_form():
    """(la, lb, lc) is the unit vector from the line to the feature, ld2 the distance, whichever way the eigenvector points:
    coeff = s (e, d) with s = 1 - 0.9 d"""
    rng = np.random.default_rng(2)
    for _ in range(20):
        u, w, n = _rot(rng).T
        c = rng.uniform(-100, 100, 3)
        t = np.array([-0.2, -0.1, 0.0, 0.1, 0.2])
        nb = c + t[:, None] * u                                        # exactly on a line
        along, d, phi = rng.uniform(-0.3, 0.3), rng.uniform(0.01, 0.5), rng.uniform(0, 2 * np.pi)
        e = np.cos(phi) * w + np.sin(phi) * n
        res = R.corner(nb[None], (c + along * u + d * e)[None])
        s = 1 - 0.9 * d
        np.testing.assert_allclose(res["coeff"][0], np.append(s * e, s * d), atol=1e-9)
        assert res["flag"][0] and abs(res["s"][0] - s) <= 1e-9
        # the neighbours in another order: the same coefficients
        res2 = R.corner(nb[::-1][None], (c + along * u + d * e)[None])
        np.testing.assert_allclose(res2["coeff"], res["coeff"], atol=1e-9)


def test_plane_of_exactly_coplanar_points():
    """n . p + d = 0 with d > 0: x = n / d, the coefficients s (n, pd2) with pd2 the feature's signed distance"""
    rng = np.random.default_rng(3)
    for _ in range(20):
        u, w, n = _rot(rng).T
        d = rng.uniform(0.5, 100.0)
        uv = rng.uniform(-0.4, 0.4, (5, 2)) + rng.uniform(-30, 30, 2)
        nb = -d * n + uv[:, :1] * u + uv[:, 1:] * w
        h = rng.uniform(-0.5, 0.5)
        sel = -d * n + uv.mean(0)[0] * u + uv.mean(0)[1] * w + h * n
        ori = rng.uniform(1.0, 80.0, 3)
        res = R.surf(nb[None], sel[None], ori[None])
        s = 1 - 0.9 * abs(h) / np.sqrt(np.linalg.norm(ori))
        assert res["rank"][0] == 3 and not res["rank_near"][0]
        np.testing.assert_allclose(res["x"][0], n / d, rtol=0, atol=1e-9 * res["cond"][0] / d)
        np.testing.assert_allclose(res["coeff"][0], np.append(s * n, s * h), atol=1e-9 * res["cond"][0])
        assert res["maxdist"][0] <= 1e-9 * res["cond"][0] and bool(res["flag"][0]) == (s > 0.1)


def test_full_rank_solution_is_the_least_squares_one():
    rng = np.random.default_rng(4)
    A = rng.normal(size=(200, 5, 3)) + rng.uniform(-20, 20, (200, 1, 3))
    b = rng.normal(size=(200, 5))
    x, rank, near, tied = R.colpiv_solve(A, b)
    assert (rank == 3).all() and not near.any() and not tied.any()
    want = np.array([np.linalg.lstsq(a, y, rcond=None)[0] for a, y in zip(A, b)])
    np.testing.assert_allclose(x, want, rtol=1e-9, atol=1e-9)


def test_rank_two_gives_the_basic_solution_not_the_minimum_norm_one():
    """five points (x_i, 10, 0.5): the y column is pivoted first, then x; z is dropped and its component is exactly zero.
    numpy's lstsq spreads the constant over y AND z (minimum norm): a different plane"""
    t = np.array([-0.25, -0.125, 0.0, 0.125, 0.25])
    nb = np.stack([5.0 + t, np.full(5, 10.0), np.full(5, 0.5)], 1)
    x, rank, near, tied = R.colpiv_solve(nb[None], -np.ones((1, 5)))
    assert rank[0] == 2 and not near[0] and not tied[0]
    assert x[0, 2] == 0.0 and abs(x[0, 0]) <= 1e-15 and abs(x[0, 1] + 0.1) <= 1e-15
    mn = np.linalg.lstsq(nb, -np.ones(5), rcond=None)[0]
    assert abs(mn[2]) > 1e-3                                            # lstsq is not what the reference calls
    res = R.surf(nb[None], np.array([[5.03, 10.125, 0.56]]), np.array([[5.03, 10.125, 0.56]]))
    assert res["flag"][0] and res["coeff"][0, 2] == 0.0 and res["maxdist"][0] <= 1e-14
    np.testing.assert_allclose(res["normal"][0], [0.0, -1.0, 0.0], atol=1e-14)
    # a column that is not dropped by a hair is reported: third pivot at twice its threshold
    nb2 = nb.copy(); nb2[:, 2] += np.array([1, -1, 1, -1, 0]) * 2.5e-6
    assert R.colpiv_solve(nb2[None], -np.ones((1, 5)))[2][0]


def test_to_map_against_float64():
    """the float32 pointAssociateToMap against the float64 rotation (ZYX, pcl::getTransformation) of the same pose"""
    rng = np.random.default_rng(5)
    p = rng.uniform(-250, 250, (500, 3)).astype(np.float32)
    got = R.to_map(S.POSE, p).astype(np.float64)
    T = S.POSE.astype(np.float64)
    want = p.astype(np.float64) @ S._rot(*T[:3]).T + T[3:]
    assert np.abs(got - want).max() <= 4 * R.f32_spacing(np.abs(want).max())
    np.testing.assert_array_equal(R.to_map(S.IDENTITY, p), p)


# ----------------------------------------------------------------------------- the scenes
def test_scene_layout():
    """build() itself checks the 3 m between neighbourhoods and the voxel diagonal between points; here: the sweeps are there"""
    sc = S.build()
    cm, sm = sc["meta"]
    for b in S.BUCKETS:
        assert ((cm["kind"] == "cross") & (cm["bucket"] == b)).sum() == 3 * len(S.RATIOS)
        assert ((sm["kind"] == "gate02") & (sm["bucket"] == b)).sum() == len(S.GATE_DIST)
        assert ((sm["kind"] == "plane") & (sm["bucket"] == b)).sum() == 4 * S.N_PLANES
    assert (sm["kind"] == "sgate").sum() == len(S.S_SWEEP)
    r = np.linalg.norm(sc["surf_q"][sm["kind"] == "sgate", :3], axis=1)
    assert r.min() >= 0.4 and r.max() <= 0.9
    c, s = S.scan(sc, S.IDENTITY)
    np.testing.assert_array_equal(c, sc["corner_q"]); np.testing.assert_array_equal(s, sc["surf_q"])


POSES = {"identity": S.IDENTITY, "posed": S.POSE}
_runs = {}


def _hand_built(pkg, lib, pose_name):
    if pose_name not in _runs:
        sc = S.build()
        h = S.load(pkg, lib, sc, POSES[pose_name])
        _runs[pose_name] = [S.designed(h, sc, POSES[pose_name], which) for which in (0, 1)]
        h.close()
    return S.build(), _runs[pose_name]


@pytest.mark.parametrize("pose_name", list(POSES))
def test_oracle_flags_on_hand_built_scenes(pkg, oracle, pose_name):
    sc, ms = _hand_built(pkg, oracle, pose_name)
    for which in (0, 1):
        m, meta = ms[which], sc["meta"][which]
        assert S.brute_force_sets(m, np.arange(len(m["sel"]))).all()
        dec = S.check_flags(f"oracle {pose_name}", which, m, meta=meta)
        S.check_gate_pairs(which, m, meta, dec, identity=(pose_name == "identity"))
        S.check_exact_cases(which, m, meta)


@pytest.mark.parametrize("pose_name", list(POSES))
def test_oracle_coefficients_on_hand_built_scenes(pkg, oracle, pose_name):
    """per class: the oracle's distance from float64, and that it stays within what float32 and the reference's own methods
    explain (S.float32_bound)"""
    sc, ms = _hand_built(pkg, oracle, pose_name)
    for which in (0, 1):
        m, meta = ms[which], sc["meta"][which]
        both = m["flag"] & m["ref"]["flag"] & np.isin(meta["kind"], S.CLASS_KINDS[which])
        cls = S.classes(which, m["ref"], both, meta["bucket"], merge=False)
        S.report_oracle_classes(f"oracle {pose_name}", which, m, cls)


def test_oracle_on_boxes(pkg, oracle):
    """make_small_scene through the staged path, then its own DS map and DS scan handed back as clouds (one point per voxel).
    At most 0.5 % of the features are undecidable (measured: 0 of 270 corner, 5 of 10 685 surf); no decidable flag differs"""
    sc = make_small_scene(pkg, oracle)
    o = pkg.LidarHotpath(oracle, **small_params())
    o.map_set(sc["map_corner"], sc["map_surf"])
    o.scan_upload(sc["scan"]); o.scan_organize(); o.scan_extract(); o.scan_downsample()
    (mc, ms), (c, s) = o.get_map_ds(), o.get_scan_ds()
    o.map_set(mc, ms)
    o.scan_to_map(c, s, sc["guess"])
    for which in (0, 1):
        m = S.measure(o, sc["guess"], which)
        assert len(m["sel"]) >= (200 if which == 0 else 8000)
        rows = np.where(m["five"])[0][::40]
        assert S.brute_force_sets(m, rows).all()
        S.check_flags("oracle boxes", which, m, cap=5e-3)
        both = m["flag"] & m["ref"]["flag"]
        cls = S.classes(which, m["ref"], both, np.full(len(both), "boxes"), merge=True)
        S.report_oracle_classes("oracle boxes", which, m, cls)
    o.close()
