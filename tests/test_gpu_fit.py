"""GPU tier (-m gpu): the per-feature coefficients of scan-to-map Gauss-Newton on the device (`corner_fit` / `corner_eval`,
`surf_fit` / `surf_eval`, `eig3_sym`, `lstsq_5x3` in csrc/lvi_icp.hip) against the float64 reference tests/fit_ref.py, on the
hand-built neighbourhoods of tests/fit_scenes.py (identity pose and one pose with every component non-zero) and on
make_small_scene ("boxes").

Both libraries get identical input: the same one-point-per-voxel map and scan clouds (boxes: the device's own DS map and DS scan
handed to both as clouds, as in test_residuals_at_fixed_pose).  Each side is judged on ITS OWN clouds, pose and debug_knn
neighbours, read back through the C ABI, by the same float64 code.

Flags: on every decidable feature (S.MARGIN) the device's flag is float64's, no allowance; which features may be undecidable
is stated per scene (S.check_flags).  Coefficients, on features flagged by the device, the oracle and float64: per feature
E_hip = max |coeff - coeff64| <= 4 max(E_orc of the class, U), direction part and distance part apart, E_orc the oracle's
largest E of the class in the same run, U the float32 spacing at the largest coordinate of the feature's neighbourhood; 4 as
in test_gpu_step.py: two float32 restatements of Jacobi and QR that order their operations differently.  No constant
tolerance in this file.  A class is a range bucket (5, 60, 250 m; boxes is one) and, for surf, a decade of cond; each holds at
least 30 features."""
import numpy as np
import pytest

import fit_ref as R
import fit_scenes as S
from helpers import bits, make_small_scene, small_params, xyzi

pytestmark = pytest.mark.gpu

POSES = {"identity": S.IDENTITY, "posed": S.POSE}
_runs = {}


def _same_inputs(mo, mg):
    """the two sides saw the same clouds and the same neighbours: the float64 results are the same numbers (an exact distance
    tie may list two neighbours in either order: the float64 sums then differ in their last bits)"""
    np.testing.assert_array_equal(bits(mo["ds"]), bits(mg["ds"]))
    np.testing.assert_array_equal(bits(mo["sel"]), bits(mg["sel"]))
    np.testing.assert_array_equal(mo["five"], mg["five"])
    f = mg["five"]
    np.testing.assert_array_equal(np.sort(mo["nb"][f].reshape(int(f.sum()), -1), 1), np.sort(mg["nb"][f].reshape(int(f.sum()), -1), 1))
    np.testing.assert_array_equal(mo["ref"]["flag"], mg["ref"]["flag"])
    ok = mg["ref"]["flag"]
    np.testing.assert_allclose(mo["ref"]["coeff"][ok], mg["ref"]["coeff"][ok], rtol=0, atol=1e-9)


def hand_built(pkg, oracle, hip, pose_name):
    """[(oracle's measure, device's measure) for corner, surf] in the order of the scene's meta arrays; once per module"""
    sc = S.build()
    if pose_name not in _runs:
        pose = POSES[pose_name]
        o, g = S.load(pkg, oracle, sc, pose), S.load(pkg, hip, sc, pose)
        for a, b in zip(o.get_map_ds() + o.get_scan_ds(), g.get_map_ds() + g.get_scan_ds()):
            np.testing.assert_array_equal(np.sort(bits(xyzi(a)[:, :3]), 0), np.sort(bits(xyzi(b)[:, :3]), 0))
        _runs[pose_name] = [(S.designed(o, sc, pose, which), S.designed(g, sc, pose, which)) for which in (0, 1)]
        o.close(); g.close()
        for mo, mg in _runs[pose_name]:
            _same_inputs(mo, mg)
    return sc, _runs[pose_name]


def boxes(pkg, oracle, hip):
    if "boxes" not in _runs:
        sc = make_small_scene(pkg, oracle)
        o = pkg.LidarHotpath(oracle, **small_params()); g = pkg.LidarHotpath(hip, **small_params())
        g.map_set(sc["map_corner"], sc["map_surf"])
        g.scan_upload(sc["scan"]); g.scan_organize(); g.scan_extract(); g.scan_downsample()
        (mcg, msg), (scg, ssg) = g.get_map_ds(), g.get_scan_ds()
        for h in (o, g):
            h.map_set(mcg, msg)
            h.scan_to_map(scg, ssg, sc["guess"])
        _runs["boxes"] = [(S.measure(o, sc["guess"], which), S.measure(g, sc["guess"], which)) for which in (0, 1)]
        o.close(); g.close()
        for mo, mg in _runs["boxes"]:
            _same_inputs(mo, mg)
    return _runs["boxes"]


def check_coefficients(name, which, mo, mg, kinds_ok, bucket, merge):
    both = mo["flag"] & mg["flag"] & mg["ref"]["flag"] & kinds_ok
    cls = S.classes(which, mg["ref"], both, bucket, merge)
    e_orc = S.class_errors(which, mo, cls)
    ed, ei = R.coeff_errors(mg["coeff"], mg["ref"])
    bad = []
    for key, v in sorted(cls.items(), key=str):
        for part, e, eo in (("direction", ed, e_orc[key][0]), ("distance", ei, e_orc[key][1])):
            bar = 4 * np.maximum(eo, mg["U"][v])
            print(f"{name} {'corner' if which == 0 else 'surf'} class {key} {part}: n {int(v.sum())}  E_hip {e[v].max():.3e}  E_orc {eo:.3e}  "
                  f"U {mg['U'][v].min():.3e} .. {mg['U'][v].max():.3e}  bar {bar.min():.3e} .. {bar.max():.3e}  E_hip/bar max {(e[v] / bar).max():.3f}")
            if not (e[v] <= bar).all():
                bad.append((key, part, float((e[v] / bar).max())))
    assert not bad, bad


# ----------------------------------------------------------------------------- hand-built neighbourhoods
@pytest.mark.parametrize("pose_name", list(POSES))
def test_flags_on_hand_built_scenes(pkg, oracle, hip, pose_name):
    """the rotated crosses (every covariance is full: eig3_sym rotates), the two exact eigenvalue ties, the tilted planes, the
    0.2 m and s > 0.1 sweeps, the rank-2 line and the plane through the origin, at 5, 60 and 250 m: the device's flag is
    float64's on every feature that is not placed at a gate by design, and so is the oracle's"""
    sc, ms = hand_built(pkg, oracle, hip, pose_name)
    for which in (0, 1):
        meta = sc["meta"][which]
        for side, m in zip(("oracle", "hip"), ms[which]):
            assert S.brute_force_sets(m, np.arange(len(m["sel"]))).all(), side
            dec = S.check_flags(f"{side} {pose_name}", which, m, meta=meta)
            S.check_gate_pairs(which, m, meta, dec, identity=(pose_name == "identity"))
            S.check_exact_cases(which, m, meta)


@pytest.mark.parametrize("pose_name", list(POSES))
def test_coefficients_on_hand_built_scenes(pkg, oracle, hip, pose_name):
    sc, ms = hand_built(pkg, oracle, hip, pose_name)
    for which in (0, 1):
        meta = sc["meta"][which]
        mo, mg = ms[which]
        check_coefficients(pose_name, which, mo, mg, np.isin(meta["kind"], S.CLASS_KINDS[which]), meta["bucket"], merge=False)


# ----------------------------------------------------------------------------- boxes
def test_flags_on_boxes(pkg, oracle, hip):
    """at most 0.5 % of the ~270 corner and ~10 700 surf features are undecidable (CPU tier: 0 and 5); on all others the
    device's flag is float64's"""
    for which, (mo, mg) in enumerate(boxes(pkg, oracle, hip)):
        assert len(mg["sel"]) >= (200 if which == 0 else 8000)
        for side, m in (("oracle", mo), ("hip", mg)):
            assert S.brute_force_sets(m, np.where(m["five"])[0][::40]).all(), side
            S.check_flags(f"{side} boxes", which, m, cap=5e-3)


def test_coefficients_on_boxes(pkg, oracle, hip):
    for which, (mo, mg) in enumerate(boxes(pkg, oracle, hip)):
        n = len(mg["sel"])
        check_coefficients("boxes", which, mo, mg, np.ones(n, bool), np.full(n, "boxes"), merge=True)
