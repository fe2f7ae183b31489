"""CPU tier of the initial two-view pose (include/lvi_relpose.h): the ABI checks, the reference
tests/relpose_ref.py on exact and on 7-point scenes (closed forms, every branch of recoverPose, solveRelativeRT and
relativePose), the same pipeline over numpy.linalg.svd and against mpmath, and csrc/lvi_relpose_math.hpp compiled alone
(plain and as a stand-alone program under the host sanitizers), which must give the reference's bits."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import fman_ref as FM
import relpose_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "lvi_relpose.h")).read()


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(lvi_relpose_[a-z0-9_]+)\s*\(", txt)))


# ---- ABI -------------------------------------------------------------------------------------------
def test_header_and_relpose_binding_agree(pkg):
    P = pkg.relpose
    assert _declared() == sorted(P.RELPOSE_SIGNATURES.keys())
    assert len(_declared()) == 10
    for other in (pkg._abi.SIGNATURES, pkg.fmat.FMAT_SIGNATURES, pkg.fman.FMAN_SIGNATURES, pkg.preint.PREINT_SIGNATURES):
        assert not set(_declared()) & set(other)
    txt = _header()
    for name, val in (("ABI_VERSION", 1), ("MIN_POINTS", P.MIN_POINTS), ("MIN_INLIERS", P.MIN_INLIERS), ("CHUNK", P.CHUNK), ("DEGENERATE", P.DEGENERATE),
                      ("NO_MODEL", P.NO_MODEL), ("TOO_FEW", P.TOO_FEW)):
        assert int(re.search(r"#define LVI_RELPOSE_%s\s+(\d+)" % name, txt).group(1)) == val, name
    assert (P.MIN_POINTS, P.MIN_INLIERS, P.WINDOW, P.MIN_PAIRS, P.FOCAL_LENGTH, P.MIN_PARALLAX_PX) == \
        (R.MIN_PAIRS_SOLVE, R.MIN_INLIERS, R.WINDOW, R.MIN_PAIRS_GATE, R.FOCAL, R.MIN_PARALLAX_PX) == (15, 12, 10, 20, 460, 30)
    assert (P.DEGENERATE, P.NO_MODEL, P.TOO_FEW) == (R.FLAG_DEGENERATE, R.FLAG_NO_MODEL, R.FLAG_TOO_FEW)
    fm = open(os.path.join(ROOT, "include", "lvi_fmat.h")).read()
    assert int(re.search(r"#define LVI_FMAT_MAX_POINTS\s+(\d+)", fm).group(1)) == P.MAX_POINTS
    assert all(s in txt for s in ("solve_5pts.cpp:193-227", "estimator.cpp:493-522", ":30-182", ":195", ":219", ":220", ":221", "estimator.cpp:502-512"))
    assert '#include "lvi_fmat.h"' in txt and "typedef struct lvi_fmat_info" not in txt                # the record is included, not copied
    for other in ("lvi_hotpath.h", "lvi_fmat.h", "lvi_fman.h", "lvi_preint.h", "lvi_win.h", "lvi_marg.h"):
        assert "lvi_relpose" not in open(os.path.join(ROOT, "include", other)).read(), other


def test_record_layouts(pkg):
    P = pkg.relpose
    txt = _header()
    for cname, cls, size in (("lvi_relpose_params", P.RelposeParams, 24), ("lvi_relpose_pose", P.RelposePose, 152)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in re.findall(r"\b(?:int32_t|double)\s+([^;]+);", body) for n in re.findall(r"([A-Za-z_][A-Za-z_0-9]*)(?:\[\d+\])?\s*(?:,|$)", decl)]
        assert names == [f[0] for f in cls._fields_], cname
        assert ctypes.sizeof(cls) == size, cname
    assert [f[0] for f in P.RelposeResult._fields_] == ["Rotation", "Translation", "average_parallax", "ok", "flags", "pose", "info"]
    assert ctypes.sizeof(P.RelposeResult) == 8 * 13 + 8 + 152 + ctypes.sizeof(pkg.fmat.FmatInfo)
    hpp = open(os.path.join(pkg.PKG_DIR, "csrc", "lvi_relpose_math.hpp")).read()
    assert "struct Pose { double R[9], t[3], sv[3]; int good[CANDIDATES], chosen, n_inliers, flags, sweeps; };" in hpp
    assert '#include "lvi_fman_math.hpp"' in hpp and "svd_null_vector(double" not in hpp             # included, not copied


def test_hip_library_exports_the_relpose_abi_and_the_oracle_does_not(pkg, oracle):
    dll = ctypes.CDLL(pkg.HIP_LIB_PATH)
    for name in _declared():
        assert hasattr(dll, name), f"{name} missing from liblvi_hip.so"
    lib = pkg.relpose.bind(pkg.load_hip())
    assert lib.dll.lvi_relpose_abi_version() == 1 and lib.dll.lvi_fmat_abi_version() == 1 and lib.dll.lvi_abi_version() == 6
    p = pkg.relpose.RelposeParams()
    lib.dll.lvi_relpose_params_default(ctypes.byref(p))
    assert (p.threshold, p.confidence, p.distance_thresh) == (R.THRESHOLD, R.CONFIDENCE, R.DIST) == (0.3 / 460, 0.99, 50.0)
    syms = subprocess.run(["nm", "-D", "--defined-only", oracle.path], capture_output=True, text=True).stdout
    assert "lvi_abi_version" in syms and "lvi_relpose_" not in syms
    b = importlib.import_module(pkg.__name__ + ".build")
    assert "lvi_relpose.hip" in b.SOURCES and os.path.join(ROOT, "include", "lvi_relpose.h") in b.hip_dependencies()
    assert pkg.RelativePose is pkg.relpose.RelativePose
    # the host mirror is header-only, outside lvi_host.hpp and the COMPONENTS table
    assert os.path.exists(os.path.join(pkg.PKG_DIR, "host", "lvi_relpose_host.hpp"))
    assert "relpose" not in open(os.path.join(pkg.PKG_DIR, "host", "lvi_host.hpp")).read() and "relpose" not in pkg.host_api.COMPONENTS


def test_average_parallax_is_a_host_function(pkg):
    """no device is needed for it, and it gives the reference's bits"""
    lib = pkg.relpose.bind(pkg.load_hip())
    for kind in ("first", "below", "above"):
        fm = FM.FeatureManager()
        FM.load(fm, R.window_frames(kind))
        pairs = np.ascontiguousarray(fm.corresponding(0, R.WINDOW), np.float64).reshape(-1, 6)
        got = lib.dll.lvi_relpose_average_parallax(pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(pairs))
        assert got == R.average_parallax(pairs)
    assert lib.dll.lvi_relpose_average_parallax(None, 0) == 0.0


def test_relative_pose_fails_loudly_without_gpu(pkg):
    """no CPU fallback: without a device the handle is refused; arguments are refused before the device is looked for"""
    import torch
    lib = pkg.load_hip()
    for bad in (dict(max_points=14), dict(max_points=pkg.relpose.MAX_POINTS + 1), dict(max_iters=0)):
        with pytest.raises(pkg.LviError) as e:
            pkg.RelativePose(lib, **bad)
        assert e.value.code == pkg._abi.LVI_ERR_INVALID_ARG
    if not torch.cuda.is_available():
        with pytest.raises(pkg.LviError) as e:
            pkg.RelativePose(lib, max_points=64)
        assert e.value.code == pkg._abi.LVI_ERR_NO_DEVICE


# ---- closed forms ------------------------------------------------------------------------------------
_ref_cache = {}


def _ref(name):
    """the reference's recover of a scene, computed once"""
    if name not in _ref_cache:
        s = R.scenes()[name]
        _ref_cache[name] = R.recover(s["E"], s["p1"], s["p2"], s["mask"])
    return _ref_cache[name]


EXACT = [f"exact{s}" for s in R.EXACT_SEEDS]
FMAT = [f"fmat{s}" for s in R.F_SEEDS]


@pytest.mark.parametrize("name", EXACT)
def test_exact_E_gives_the_true_motion(name):
    s, r = R.scenes()[name], _ref(name)
    Rm, t = np.array(r["R"]), np.array(r["t"])
    assert np.abs(Rm - s["R"]).max() < 1e-6 and np.abs(t - s["t"] / np.linalg.norm(s["t"])).max() < 1e-6     # the points are float32
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Rm) - 1) < 1e-14 and abs(np.linalg.norm(t) - 1) < 1e-14
    tx = R.skew(t) @ Rm
    k = np.vdot(tx, s["E"]) / np.vdot(tx, tx)
    assert np.abs(k * tx - s["E"]).max() < 1e-14 * np.abs(s["E"]).max() * 10
    assert r["flags"] == 0 and r["n_inliers"] == max(r["good"]) and abs(r["sv"][0] - r["sv"][1]) < 1e-14 and r["sv"][2] < 1e-15
    # the winner keeps the points that lie within 50 baselines of both cameras, and only those
    X = np.c_[s["p1"].astype(np.float64), np.ones(len(s["p1"]))] * R.two_view(int(name[5:]), len(s["p1"]))[5][:, None]
    far = np.maximum(X[:, 2], (X @ s["R"].T + s["t"])[:, 2]) / np.linalg.norm(s["t"])
    assert (far < 49.9).sum() <= r["n_inliers"] <= (far < 50.1).sum() and r["n_inliers"] >= 0.5 * len(far)
    assert sorted(r["good"])[2] == 0


@pytest.mark.parametrize("name", FMAT)
def test_seven_point_F_gives_a_rotation_and_a_unit_translation(name):
    s, r = R.scenes()[name], _ref(name)
    Rm, t = np.array(r["R"]), np.array(r["t"])
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Rm) - 1) < 1e-14 and abs(np.linalg.norm(t) - 1) < 1e-14
    assert r["sv"][0] > r["sv"][1] > 1e3 * r["sv"][2]                      # rank 2 with unequal singular values: the case that matters
    assert t @ s["E"] / r["sv"][0] == pytest.approx(np.zeros(3), abs=1e-9)  # t is the left null vector
    assert R.MIN_INLIERS < r["n_inliers"] <= int(np.asarray(s["mask"]).sum()) and not (r["mask"] & ~np.asarray(s["mask"])).any()


def _canon(cands):
    """the candidate set without its order: sorted rounded (R, t) tuples"""
    return sorted(tuple(np.round(np.r_[np.ravel(Rc), np.ravel(tc)], 9) + 0.0) for Rc, tc in cands)


@pytest.mark.parametrize("name", EXACT[:4] + FMAT[:4])
def test_candidate_set_is_invariant_under_sign_and_scale(name):
    s = R.scenes()[name]
    base = _canon(_ref(name)["cand"])
    for k in (-1.0, 1e-3):
        r = R.recover(k * np.asarray(s["E"]), s["p1"], s["p2"], s["mask"])
        assert _canon(r["cand"]) == base
        assert np.abs(np.array(r["R"]) - _ref(name)["R"]).max() < 1e-9 and np.abs(np.array(r["t"]) - _ref(name)["t"]).max() < 1e-9     # the same winner
        assert r["n_inliers"] == _ref(name)["n_inliers"]


def test_every_candidate_wins_somewhere():
    winners = {}
    for name in EXACT + FMAT:
        winners.setdefault(_ref(name)["chosen"], []).append(name)
    print("[relpose ref] winners:", {k: len(v) for k, v in sorted(winners.items())})
    assert sorted(winners) == [0, 1, 2, 3]


# ---- branches ------------------------------------------------------------------------------------------
def _branch(name):
    s = R.branch_scenes()[name]
    return s, R.recover(s["E"], s["p1"], s["p2"], s["mask"], s["dist"])


def test_zero_mask_gives_candidate_zero():
    s, r = _branch("zero_mask")
    assert r["good"] == [0, 0, 0, 0] and r["chosen"] == 0 and r["n_inliers"] == 0 and r["flags"] == 0 and not r["masks"].any()
    assert np.array_equal(r["R"], r["cand"][0][0]) and np.array_equal(r["t"], r["cand"][0][1])


def test_planted_tie_gives_the_earlier_candidate():
    s, r = _branch("tie")
    top = sorted(r["good"], reverse=True)
    assert top[0] == top[1] == 9 and top[2] == 0
    assert r["chosen"] == r["good"].index(9) and r["good"].index(9) < 3 and r["good"][r["chosen"] + 1:].count(9) == 1


def test_distance_threshold_and_parallel_rays():
    s, r = _branch("planted")
    D = R.decompose(s["E"].tolist())
    assert (np.array(D["R1"]) == np.eye(3)).all() and D["t"] == [1.0, 0.0, 0.0]              # the construction is exact
    Q, _ = R.svd_null_vector(R.triangulation_matrix(R.candidate(D, 0), 0.0, 0.0, 0.0, 0.0))
    assert Q == [0.0, 0.0, 1.0, 0.0]                                                          # Q3 == 0
    assert r["chosen"] == 0 and r["mask"][:3].tolist() == [0, 0, 1] and r["masks"][:, 0].tolist() == [0, 0, 0, 0]
    assert r["n_inliers"] == len(s["p1"]) - 2 and np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all()
    # the threshold is a parameter: at 100 the point at 80 baselines passes, the parallel rays never do
    far = R.recover(s["E"], s["p1"], s["p2"], None, 100.0)
    assert far["mask"][:3].tolist() == [0, 1, 1]
    s, near = _branch("near")
    assert 0 < near["n_inliers"] < R.recover(s["E"], s["p1"], s["p2"])["n_inliers"]


@pytest.mark.parametrize("name", ["E_zero", "E_rank1", "E_nan", "E_inf", "E_huge"])
def test_degenerate_E_is_no_pose(name):
    s, r = _branch(name)
    assert r["flags"] == R.FLAG_DEGENERATE and r["good"] == [0, 0, 0, 0] and r["chosen"] == 0 and not r["masks"].any()
    assert (np.array(r["R"]) == np.eye(3)).all() and r["t"] == [0.0, 0.0, 0.0] and r["sv"] == [0.0, 0.0, 0.0]


def test_a_rank_one_E_in_general_position_stays_finite():
    """its second singular value is rounding noise, not 0: a pose comes out, and no NaN"""
    s, r = _branch("E_outer")
    assert r["flags"] == 0 and 0 < r["sv"][1] < 1e-15 and np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all()


@pytest.mark.parametrize("n, ok", [(14, False), (15, True)])
def test_solve_relative_rt_wants_fifteen_pairs(n, ok):
    p1, p2, *_ = R.two_view(60, n)
    r = R.solve_relative_rt(R.pairs_of(p1, p2))
    assert r["ok"] is ok and r["flags"] == (0 if ok else R.FLAG_TOO_FEW)
    if ok:
        assert r["pose"]["n_inliers"] > R.MIN_INLIERS
        Rm, t = np.array(r["pose"]["R"]), np.array(r["pose"]["t"])
        assert np.array_equal(np.array(r["Rotation"]), Rm.T) and np.abs(np.array(r["Translation"]) + Rm.T @ t).max() < 1e-15


@pytest.mark.parametrize("k, ok", [(12, False), (13, True)])
def test_solve_relative_rt_wants_more_than_twelve_inliers(k, ok):
    pairs, status, E = R.inlier_scene(k)
    r = R.solve_relative_rt(pairs, model=(status, E, 0))
    assert r["pose"]["n_inliers"] == k and r["ok"] is ok and np.isfinite(r["Rotation"]).all()


def test_no_model_is_not_a_pose():
    k = np.arange(40)
    p1 = np.c_[(50 + 8 * k) / 460.0, (100 + 2 * k) / 460.0]
    r = R.solve_relative_rt(R.pairs_of(p1, p1 + 3 / 460.0))
    assert r["flags"] == R.FLAG_NO_MODEL and not r["ok"] and r["pose"] is None and (np.array(r["Rotation"]) == np.eye(3)).all()


def _window(kind):
    fm = FM.FeatureManager()
    FM.load(fm, R.window_frames(kind))
    return R.relative_pose(fm.corresponding)


def test_relative_pose_wants_more_than_twenty_pairs():
    ok, l, _, _, recs = _window("pairs20")
    assert not ok and l == -1 and len(recs) == R.WINDOW and all(r["n"] == 20 and r["average_parallax"] is None for r in recs)
    ok, l, _, _, recs = _window("pairs21")
    assert ok and l == 0 and recs[0]["n"] == 21 and recs[0]["solved"]


def test_relative_pose_parallax_gate():
    ok, l, _, _, recs = _window("below")
    px = recs[0]["average_parallax"] * R.FOCAL
    assert not ok and 30 * (1 - 2e-9) < px < 30 and not any(r["solved"] for r in recs)
    ok, l, Rot, T, recs = _window("above")
    px = recs[0]["average_parallax"] * R.FOCAL
    assert ok and l == 0 and 30 < px < 30 * (1 + 2e-9) and recs[0]["solved"]
    assert np.abs(np.array(Rot) - np.eye(3)).max() < 1e-5 and abs(abs(T[0]) - 1) < 1e-6                  # a pure translation along x


def test_relative_pose_takes_the_first_frame_that_passes():
    assert _window("first")[:2] == (True, 0)
    ok, l, Rot, T, recs = _window("third")
    assert ok and l == 3 and [r["solved"] for r in recs] == [False, False, False, True] and [r["n"] for r in recs] == [25, 25, 25, 40]
    ok, l, Rot, T, recs = _window("garbage")
    assert ok and l == 3 and [(r["solved"], r["ok"]) for r in recs] == [(True, False)] * 3 + [(True, True)]
    assert np.array_equal(Rot, recs[3]["result"]["Rotation"])


def test_relative_pose_when_none_passes():
    ok, l, Rot, T, recs = _window("still")
    assert not ok and l == -1 and len(recs) == R.WINDOW and not any(r["solved"] for r in recs)
    assert (np.array(Rot) == np.eye(3)).all() and T == [0.0, 0.0, 0.0]


# ---- the independent route and mpmath -------------------------------------------------------------------
def _same_pose(a, b):
    return np.abs(np.array(a["R"]) - np.array(b["R"])).max() < 1e-9 and np.abs(np.array(a["t"]) - np.array(b["t"])).max() < 1e-9


def test_numpy_svd_route_gives_the_same_winner_and_mask():
    """the winner as a pose, since the conventions of an SVD permute the four candidates among themselves"""
    aside, names = 0, EXACT + FMAT
    for name in names:
        s, a = R.scenes()[name], _ref(name)
        b = R.recover(s["E"], s["p1"], s["p2"], s["mask"], route="numpy")
        top = sorted(b["good"], reverse=True)
        if top[0] == top[1] or not b["margin"] > 1e-9:
            aside += 1
            continue
        assert _same_pose(a, b) and np.array_equal(a["mask"], b["mask"]) and sorted(a["good"]) == sorted(b["good"]), name
    print(f"[relpose ref] numpy route: {len(names)} scenes, {aside} set aside")
    assert aside <= 0.05 * len(names)


@pytest.mark.parametrize("name", EXACT + FMAT)
def test_pose_against_mpmath(name):
    """the bar is §26's: 10 G of that scene, never below 16 ulp; G is the numpy-SVD route's distance from mpmath"""
    s, a = R.scenes()[name], _ref(name)
    b = R.decompose_numpy(s["E"])
    exact = R.candidates_mp(s["E"])
    G = max(R.pose_dev(b["R1"], b["t"], exact), R.pose_dev(b["R2"], b["t"], exact))
    own = max(R.pose_dev(Rc, tc, exact) for Rc, tc in a["cand"])
    print(f"[relpose ref] {name}: G {G:.3e}, bar {R.pose_bar(G):.3e}, the reference's distance from mpmath {own:.3e}, sweeps {a['sweeps']}")
    assert own <= R.pose_bar(G) and 1 <= a["sweeps"] < R.MAX_SWEEPS


# ---- csrc/lvi_relpose_math.hpp alone, plain and under the host sanitizers ------------------------------------------
DRIVER = r"""
// stand-alone driver of csrc/lvi_relpose_math.hpp: recoverPose, the pose inversion and the parallax, run on the host
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lvi_relpose_math.hpp"
using namespace lvi_relpose_math;
static void hex(const double* v, int n) { for (int k = 0; k < n; k++) printf("%a ", v[k]); }
int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    double head[13];
    while (fread(head, sizeof(double), 13, f) == 13) {
        const int kind = (int)head[0], n = (int)head[1], has_mask = (int)head[2];
        if (n < 1 || n > 100000) return 4;
        if (kind == 0) {                                   // recover: E = head[4..12], dist = head[3]
            std::vector<double> xy(4 * (size_t)n), m(n);
            if (fread(xy.data(), sizeof(double), xy.size(), f) != xy.size() || fread(m.data(), sizeof(double), n, f) != (size_t)n) return 5;
            std::vector<float> pts(xy.begin(), xy.end());
            std::vector<unsigned char> in(n), masks(4 * (size_t)n);
            for (int k = 0; k < n; k++) in[k] = m[k] != 0;
            Pose p;
            double cand[4][12];
            recover_serial(head + 4, pts.data(), has_mask ? in.data() : nullptr, n, head[3], p, cand, masks.data());
            hex(p.R, 9); hex(p.t, 3); hex(p.sv, 3);
            printf("%d %d %d %d %d %d %d %d ", p.good[0], p.good[1], p.good[2], p.good[3], p.chosen, p.n_inliers, p.flags, p.sweeps);
            hex(&cand[0][0], 48);
            for (size_t k = 0; k < masks.size(); k++) putchar('0' + masks[k]);
            double Rot[9], T[3];
            invert_pose(p.R, p.t, Rot, T);
            putchar(' '); hex(Rot, 9); hex(T, 3);
            putchar('\n');
        } else {                                           // average_parallax of pairs [n][6]
            std::vector<double> pairs(6 * (size_t)n);
            if (fread(pairs.data(), sizeof(double), pairs.size(), f) != pairs.size()) return 6;
            printf("%a\n", average_parallax(pairs.data(), n));
        }
    }
    fclose(f);
    return 0;
}
"""


def _build_driver(pkg, d, flags):
    d.mkdir()
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", *flags, "-I" + os.path.join(pkg.PKG_DIR, "csrc"), "-o", str(exe),
                        str(d / "driver.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.fixture(scope="module")
def drivers(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("relpose_header")
    return {"plain": _build_driver(pkg, d / "plain", []),
            "san": _build_driver(pkg, d / "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])}


def _recover_blob(s, dist):
    n = len(s["p1"])
    m = np.ones(n) if s["mask"] is None else np.asarray(s["mask"], np.float64)
    xy = np.c_[np.asarray(s["p1"], np.float32), np.asarray(s["p2"], np.float32)].astype(np.float64)
    return np.r_[0.0, float(n), 0.0 if s["mask"] is None else 1.0, float(dist), np.asarray(s["E"], np.float64).ravel(), xy.ravel(), m].tobytes()


def _header_cases():
    """every scene of this file: (name, blob, the reference's result)"""
    out = []
    for name, s in R.scenes().items():
        out.append((name, _recover_blob(s, R.DIST), _ref(name)))
    for name, s in R.branch_scenes().items():
        out.append((name, _recover_blob(s, s["dist"]), R.recover(s["E"], s["p1"], s["p2"], s["mask"], s["dist"])))
    for k in (12, 13):
        pairs, status, E = R.inlier_scene(k)
        p1, p2 = R.pair_points(pairs)
        out.append((f"inliers{k}", _recover_blob(dict(E=E, p1=p1, p2=p2, mask=status), R.DIST), R.recover(E, p1, p2, status)))
    return out


@pytest.mark.parametrize("which", ["plain", "san"])
def test_math_header_gives_the_reference_bits(drivers, tmp_path, which):
    """R, t, the singular values, the four counts, the choice, the flags, the four candidates and the four masks, and the
    inverted pose, bit for bit on every scene; the sanitizer build must exit clean"""
    cases = _header_cases()
    windows = []
    for kind in R.WINDOWS:
        fm = FM.FeatureManager()
        FM.load(fm, R.window_frames(kind))
        for i in (0, 3):
            pairs = np.asarray(fm.corresponding(i, R.WINDOW), np.float64).reshape(-1, 6)
            if len(pairs):
                windows.append(pairs)
    blob = b"".join(c[1] for c in cases) + b"".join(np.r_[1.0, float(len(p)), np.zeros(11), p.ravel()].tobytes() for p in windows)
    (tmp_path / "s.bin").write_bytes(blob)
    out = subprocess.run([drivers[which], str(tmp_path / "s.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l.split() for l in out.stdout.split("\n") if l]
    assert len(lines) == len(cases) + len(windows)
    for (name, _, r), tok in zip(cases, lines):
        n = r["masks"].shape[1]
        val = [float.fromhex(v) for v in tok[:15]]
        ints = [int(v) for v in tok[15:23]]
        cand = [float.fromhex(v) for v in tok[23:71]]
        masks = np.array([int(ch) for ch in tok[71]], np.uint8).reshape(4, n)
        inv = [float.fromhex(v) for v in tok[72:84]]
        want = np.r_[np.ravel(r["R"]), r["t"], r["sv"]]
        assert np.array_equal(np.array(val).view(np.uint64), want.view(np.uint64)), name
        assert ints == r["good"] + [r["chosen"], r["n_inliers"], r["flags"], r["sweeps"]], name
        wc = np.concatenate([np.r_[np.ravel(Rc), tc] for Rc, tc in r["cand"]])
        assert np.array_equal(np.array(cand).view(np.uint64), wc.view(np.uint64)), name
        assert np.array_equal(masks, r["masks"]), name
        Rot, T = R.invert_pose(r["R"], r["t"])
        assert np.array_equal(np.array(inv).view(np.uint64), np.r_[np.ravel(Rot), T].view(np.uint64)), name
    for pairs, tok in zip(windows, lines[len(cases):]):
        assert float.fromhex(tok[0]) == R.average_parallax(pairs)
    print(f"[relpose header] {which}: {len(cases)} scenes and {len(windows)} pair lists, every bit equal")
