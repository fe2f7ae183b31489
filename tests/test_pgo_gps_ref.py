"""CPU tier of the GPS factors and the marginal covariance of the pose graph (include/lvi_pgo_gps.h): the ABI
and binding checks, the float64 reference tests/pgo_gps_ref.py against central differences, known answers and itself
(two linear solvers, two covariance routes), the conditions the GPU tier relies on, and the two host pieces compiled alone
into stand-alone programs, plain and under the host sanitizers: the GPS error of csrc/lvi_pgo_math.hpp and the decision of
host/lvi_gps_gate.hpp."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import pgo_gps_ref as GR
import pgo_ref as R
import test_pgo_ref as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lvi_pgo_gps.h")
FLOOR = 10 * R.CONV_EPS


def _declared(path=HEADER):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lvi_pgo_[a-z0-9_]+)\s*\(", txt)))


# ---- ABI -------------------------------------------------------------------------------------------
def test_header_and_gps_binding_agree(pkg):
    assert _declared() == sorted(pkg.pgo.PGO_GPS_SIGNATURES) == ["lvi_pgo_gps_abi_version", "lvi_pgo_gps_add", "lvi_pgo_gps_count", "lvi_pgo_gps_marginal_covariance"]
    # a separate table and a separate header: lvi_pgo.h keeps its 11
    assert len(pkg.pgo.PGO_SIGNATURES) == 11 and not set(pkg.pgo.PGO_SIGNATURES) & set(pkg.pgo.PGO_GPS_SIGNATURES)
    assert len(_declared(os.path.join(ROOT, "include", "lvi_pgo.h"))) == 11
    assert not set(_declared()) & set(pkg._abi.SIGNATURES)
    txt = open(HEADER).read()
    assert int(re.search(r"#define LVI_PGO_GPS_ABI_VERSION\s+(\d+)", txt).group(1)) == 1
    # every declaration cites the reference lines it replaces
    assert all(s in txt for s in (":1430-1507", ":1497-1499", ":1591", ":1546-1566"))
    # the files that said "GPS factors are not restated" point here now
    for rel in ("include/lvi_pgo.h", "lidar-visual-inertial-slam_amd/host/lvi_pgo_host.hpp", "lidar-visual-inertial-slam_amd/host/lvi_host.hpp",
                "lidar-visual-inertial-slam_amd/host/ros2/map_optimization_node.cpp", "lidar-visual-inertial-slam_amd/pgo.py"):
        body = open(os.path.join(ROOT, rel)).read()
        assert "not restated" not in body and "GPS factors are out of scope" not in body, rel
        assert "lvi_pgo_gps.h" in body or "lvi_gps_gate.hpp" in body, rel
    # both libraries are rebuilt when the header changes
    build = importlib.import_module(pkg.__name__ + ".build")
    assert HEADER in build.hip_dependencies() and HEADER in pkg.host_api.host_dependencies(pkg.host_api.component_sources(["pgo"]))


def test_hip_library_exports_the_gps_abi_and_the_oracle_does_not(pkg, oracle):
    dll = ctypes.CDLL(pkg.HIP_LIB_PATH)
    for name in _declared():
        assert hasattr(dll, name), f"{name} missing from liblvi_hip.so"
    lib = pkg.pgo.bind(pkg.load_hip())
    assert lib.dll.lvi_pgo_gps_abi_version() == 1
    assert lib.dll.lvi_pgo_abi_version() == 1
    assert lib.dll.lvi_abi_version() == 6
    syms = subprocess.run(["nm", "-D", "--defined-only", oracle.path], capture_output=True, text=True).stdout
    assert "lvi_abi_version" in syms and "lvi_pgo_" not in syms
    H = pkg.host_api
    host = subprocess.run(["nm", "-D", "--defined-only", H.HOST_HIP_LIB], capture_output=True, text=True).stdout
    for name in ("lvh_seq_use_gps", "lvh_seq_gps_push", "lvh_seq_gps_last"):
        assert re.search(r"\b%s\b" % name, host), name
    # without a handle the calls refuse, they do not crash
    assert lib.dll.lvi_pgo_gps_add(None, 0, None, None) == pkg._abi.LVI_ERR_INVALID_ARG
    assert lib.dll.lvi_pgo_gps_count(None, None) == pkg._abi.LVI_ERR_INVALID_ARG
    assert lib.dll.lvi_pgo_gps_marginal_covariance(None, 0, None) == pkg._abi.LVI_ERR_INVALID_ARG


def test_gps_yaml_defaults(pkg, tmp_path):
    """utility.h:178-183: a parameter file that sets none of the three takes the declared defaults; one that does is read"""
    p = tmp_path / "params.yaml"
    p.write_text("/**:\n  ros__parameters:\n    gpsTopic: \"odometry/gpsz\"\n    N_SCAN: 6\n")
    assert pkg.config.load_gps_yaml(str(p)) == dict(use_gps_elevation=False, gps_cov_threshold=2.0, pose_cov_threshold=25.0, gps_topic="odometry/gpsz")
    p.write_text("/**:\n  ros__parameters:\n    useGpsElevation: true\n    gpsCovThreshold: 3\n    poseCovThreshold: 12.5\n")
    assert pkg.config.load_gps_yaml(str(p)) == dict(use_gps_elevation=True, gps_cov_threshold=3.0, pose_cov_threshold=12.5, gps_topic="lio_sam/odometry/gps")


# ---- the reference itself ------------------------------------------------------------------------------
def _central3(f):
    J = np.zeros((3, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = TP.H_CD
        J[:, k] = (f(d) - f(-d)) / (2 * TP.H_CD)
    return J


def test_gps_jacobian_against_central_differences():
    """the same h and the same bound as test_pgo_ref.py derives for the other factors (errors of size <= 4 here too)"""
    worst = 0.0
    rs = np.random.RandomState(8)
    for full in (1, 0):
        for Xi, Xj, _ in TP._cases():
            for X in (Xi, Xj):
                z = X[:3, 3] + rs.normal(0, 1, 3)
                r, J = GR.gps_error(X, z)
                assert np.abs(r).max() <= 4.0 * 1.5
                worst = max(worst, np.abs(J - _central3(lambda d: GR.gps_error(X @ R.pose_exp(d, full), z)[0])).max())
    print(f"[pgo gps ref] GPS Jacobian vs central differences (h = {TP.H_CD}): {worst:.3e}")
    assert worst <= TP.JAC_GAP_BOUND


def test_refused_gps_factors():
    g = R.build(R.scene(5, [], 1), GR.GpsGraph())
    for key, z, v in ((-1, [1, 2, 3], [1, 1, 1]), (5, [1, 2, 3], [1, 1, 1]), (2, [np.nan, 0, 0], [1, 1, 1]), (2, [1, 2, 3], [0, 1, 1]), (2, [1, 2, 3], [1, -1, 1]),
                      (2, [1, 2, 3], [1, 1, np.inf])):
        with pytest.raises(ValueError):
            g.add_gps(key, z, v)
    assert g.gps_count() == 0


def test_exact_gps_fixes_return_ground_truth():
    """exact odometry and exact fixes on a chain whose initial estimate was moved as a whole: the prior (weak: 1e8 on the
    translation) gives way and the fixes pull every key back; a graph without GPS steps exactly as pgo_ref's"""
    n = 12
    gt = [R.pose_from_rpyxyz(R.pose_to_rpyxyz(T)) for T in R.trajectory(n, 3)]
    for full in (1, 0):
        for solver in ("lstsq", "chol"):
            g = GR.GpsGraph(full, max_iters=GR.GPS_MAX_ITERS)
            for k in range(n):
                g.add_pose(None if k == 0 else R.pose_to_rpyxyz(gt[k - 1]), R.pose_to_rpyxyz(gt[k]))
            for k in (0, 5, 11):
                g.add_gps(k, gt[k][:3, 3], [1, 1, 1])
            zs = [z for _, z, _ in g.gps]
            shift = R.pose_exp(np.r_[0.0, 0.0, 0.05, 0.3, -0.2, 0.1])
            g.X = [shift @ x for x in g.X]
            info = g.solve(solver)
            # the fixes are float casts of the truth: the minimiser sits within their rounding (8 m x 2^-24) of it
            err = max(np.abs(x[:3, 3] - t[:3, 3]).max() for x, t in zip(g.X, gt))
            print(f"[pgo gps ref] exact fixes, full_logmap {full}, {solver}: iterations {info['iterations']}, chi2 {info['chi2_before']:.3e} -> {info['chi2_after']:.3e}, "
                  f"|t - truth| {err:.3e}; fix rounding {max(np.abs(z - gt[k][:3, 3]).max() for z, k in zip(zs, (0, 5, 11))):.3e}")
            assert info["converged"] and info["chi2_before"] > 1e-2 and err < 1e-5
    sc = R.gpu_scene("n37")
    a, b = R.build(sc, R.Graph(1)), R.build(sc, GR.GpsGraph(1))
    ia, ib = a.solve("chol"), b.solve("chol")
    assert ia == ib and np.array_equal(a.poses(), b.poses())


# ---- the GPU tier's scenes ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solved():
    """(scene, full_logmap) -> (scene dict, graph at the lstsq answer, lstsq poses, info, chol poses, info), computed once"""
    cache = {}

    def get(name, full):
        if (name, full) not in cache:
            sc = GR.gps_scene(name)
            g = GR.build(sc, GR.GpsGraph(full, max_iters=GR.GPS_MAX_ITERS))
            (Xa, ia), (Xb, ib) = GR.solve_both(g)
            cache[(name, full)] = (sc, g, Xa, ia, Xb, ib)
        return cache[(name, full)]
    return get


def test_gps_scene_shapes():
    S = GR.GPS_SCENES
    assert list(S) == ["g5", "g12", "g20_mid", "g37_key0", "g37_twice", "g64", "g300"]
    assert [S[k][0] for k in S] == [5, 12, 20, 37, 37, 64, "n300"]
    assert S["g5"][1] == [] and S["g12"][1] == [(11, 0)] and S["g20_mid"][1] == [(19, 2)] and S["g37_key0"][1] == R.GPU_SCENES["n37"][1]
    assert S["g37_twice"][1] == [(36, 0)] and S["g64"][1] == [(63, 1), (40, 7)]
    assert [S[k][2] for k in list(S)[:6]] == [[4], [11], [10], [0], [36, 36], [20, 63]]
    k300 = S["g300"][2]
    assert k300[:3] == [100, 200, 299] and k300[3:] == list(range(0, 300, 7)) and len(set(k300)) == len(k300)
    for name in S:
        sc = GR.gps_scene(name)
        assert [k for k, _, _ in sc["gps"]] == S[name][2]
        for k, z, v in sc["gps"]:
            assert z.dtype == np.float32 and v.dtype == np.float32 and list(v) == [1.0, 2.0, 1.0]
            assert np.abs(z - sc["gt"][k][:3, 3]).max() < 5 * GR.GPS_SIGMA
    assert len(GR.gps_scene("g300")["poses"]) == 300 and len(GR.gps_scene("g300")["loops"]) == 5
    a, b = GR.gps_scene("g64"), GR.gps_scene("g64")
    assert all(np.array_equal(x[1], y[1]) for x, y in zip(a["gps"], b["gps"]))        # seeded


@pytest.mark.parametrize("name", list(GR.GPS_SCENES))
def test_gps_scenes_converge_with_both_solvers(solved, name):
    """what tests/test_gpu_pgo_gps.py relies on, met by the reference alone: both linear solvers below conv_eps within the
    scene's max_iters (30), at a distance G far below the floor of the GPU tier's tolerance"""
    for full in (1, 0):
        sc, g, Xa, ia, Xb, ib = solved(name, full)
        gr, gt = GR.abs_gaps(Xa, Xb)
        print(f"[pgo gps ref] {name} full_logmap {full}: iterations {ia['iterations']} / {ib['iterations']}, steps {['%.1e' % s for s in ia['steps']]}, "
              f"G absolute ({gr:.3e}, {gt:.3e}), chi2 {ia['chi2_before']:.6g} -> {ia['chi2_after']:.9g}")
        for info in (ia, ib):
            assert info["converged"] and info["iterations"] <= GR.GPS_MAX_ITERS and info["max_step"] < R.CONV_EPS, (name, full, info["steps"])
            assert info["chi2_after"] < info["chi2_before"]
        assert max(gr, gt) < FLOOR
    if name == "g64":
        # undamped Gauss-Newton on this scene converges linearly: more steps than the default max_iters, the tenth far above conv_eps
        _, _, _, ia, _, _ = solved("g64", 1)
        assert ia["iterations"] > R.MAX_ITERS + 1 and ia["steps"][R.MAX_ITERS - 1] > 10 * R.CONV_EPS


@pytest.mark.parametrize("name", list(GR.GPS_SCENES))
def test_covariance_routes_agree_with_gps(solved, name):
    """QR of the whitened Jacobian against the Cholesky inverse of the normal equations, last key, both charts"""
    for full in (1, 0):
        sc, g, *_ = solved(name, full)
        last = len(g.X) - 1
        Ca, Cb = g.marginal_covariance(last, "qr"), g.marginal_covariance(last, "chol")
        gap = GR.cov_gap(Ca, Cb)
        print(f"[pgo gps ref] covariance {name} full_logmap {full}, key {last}: G_cov {gap:.3e} relative to max|C| = {np.abs(Ca).max():.6g}; "
              f"(3,3) {Ca[3, 3]:.6g}, (4,4) {Ca[4, 4]:.6g}")
        assert gap < 1e-7                                                 # so the GPU tier's tolerance max(10 G_cov, 1e-9) stays below 1e-6
        assert np.abs(Ca - Ca.T).max() <= 1e-12 * np.abs(Ca).max() and (np.diag(Ca) > 0).all()
        if name == "g20_mid":
            assert Ca[3, 3] > 25.0 and Cb[3, 3] > 25.0                    # weak yaw about the fix x lever arm: the gate stays open
        else:
            assert Ca[3, 3] < 25.0 and Ca[4, 4] < 25.0


@pytest.mark.parametrize("name", ["n37", "n300"])
def test_covariance_routes_agree_without_gps_and_the_plain_inverse_does_not(name):
    """QR against the gauge split, keys first / middle / last, both charts; and the measurement behind the split: inv(J'J) of
    a system that holds 1e-8 beside 1e6 is off by 1e-3 and more"""
    sc = R.gpu_scene(name)
    for full in (1, 0):
        g = R.build(sc, GR.GpsGraph(full))
        assert g.solve("lstsq")["converged"]
        n = len(g.X)
        for key in (0, n // 2, n - 1):
            Cq, Cs, Ci = (g.marginal_covariance(key, r) for r in ("qr", "split", "inv"))
            gs, gi = GR.cov_gap(Cq, Cs), GR.cov_gap(Cq, Ci)
            print(f"[pgo gps ref] covariance {name} without GPS, full_logmap {full}, key {key}: split vs QR {gs:.3e}, inv(J'J) vs QR {gi:.3e}, max|C| {np.abs(Cq).max():.6g}")
            assert gs < 1e-7 and gi > 1e-4 and gi > 1e3 * gs
        with pytest.raises(ValueError):
            GR.build(GR.gps_scene("g5"), GR.GpsGraph(full)).marginal_covariance(0, "split")


def test_covariance_of_one_key_is_its_prior():
    for full in (1, 0):
        g = GR.GpsGraph(full)
        g.add_pose(None, np.float32([0.1, -0.2, 2.5, 30.0, -12.0, 1.5]))
        for route in ("split", "qr", "chol"):
            C = g.marginal_covariance(0, route)
            assert np.abs(C - np.diag(R.PRIOR_VAR)).max() <= 1e-9 * 1e8, route


# ---- stand-alone host programs ---------------------------------------------------------------------------
def _compile(d, name, source, includes, flags):
    d.mkdir(parents=True, exist_ok=True)
    (d / (name + ".cpp")).write_text(source)
    exe = d / name
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", *flags, *["-I" + i for i in includes], "-o", str(exe),
                        str(d / (name + ".cpp"))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

MATH_DRIVER = r"""
// stand-alone driver of the GPS pieces of csrc/lvi_pgo_math.hpp, run on the host
#include <cstdio>
#include "lvi_pgo_math.hpp"
using namespace lvi_pgo_math;

int main(int argc, char** argv)
{
    if (argc < 2) return 1;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    double rec[19];                      // X as a 4x4, z [3]
    while (std::fread(rec, 8, 19, f) == 19) {
        Pose X;
        pose_from_matrix(rec, &X);
        double r[3], J[18];
        gps_error(X, rec + 16, r, J);
        for (int i = 0; i < 3; i++) std::printf(" %a", r[i]);
        for (int i = 0; i < 18; i++) std::printf(" %a", J[i]);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
"""


@pytest.mark.parametrize("which", ["plain", "san"])
def test_math_header_gps_error_equals_the_reference(pkg, tmp_path, which):
    exe = _compile(tmp_path / which, "gps_math", MATH_DRIVER, [os.path.join(pkg.PKG_DIR, "csrc")], SAN if which == "san" else [])
    tol = 4.0 * TP.jacobian_gap()                                         # the bound test_pgo_ref.py uses for the other factors
    rs = np.random.RandomState(9)
    blob, want = b"", []
    for Xi, Xj, _ in TP._cases():
        for X in (Xi, Xj):
            z = X[:3, 3] + rs.normal(0, 1, 3)
            blob += np.r_[X.ravel(), z].astype(np.float64).tobytes()
            r, J = GR.gps_error(X, z)
            want.append(np.r_[r, J.ravel()])
    (tmp_path / "g.bin").write_bytes(blob)
    out = subprocess.run([exe, str(tmp_path / "g.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [np.array([float.fromhex(x) for x in l.split()]) for l in out.stdout.split("\n") if l]
    assert len(got) == len(want) == 40
    worst = max(np.abs(a - b).max() for a, b in zip(got, want))
    print(f"[pgo gps header] {which}: GPS error and Jacobian vs reference {worst:.3e} (tolerance {tol:.3e})")
    assert 0 < tol < 4 * TP.JAC_GAP_BOUND and worst <= tol


GATE_DRIVER = r"""
// stand-alone driver of host/lvi_gps_gate.hpp: a script of commands, one answer line per "add"
//   reset elev gpsCov poseCov | push stamp x y z cx cy cz | add t fx fy fz bx by bz covxx covyy z | addnokeys t covxx covyy z
#include <cstdio>
#include <cstring>
#include "lvi_gps_gate.hpp"
using namespace lvi_host;

int main(int argc, char** argv)
{
    if (argc < 2) return 1;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    GpsGate* g = new GpsGate();
    char cmd[32];
    while (std::fscanf(f, "%31s", cmd) == 1) {
        if (!std::strcmp(cmd, "reset")) {
            int e; float a, b;
            if (std::fscanf(f, "%d %f %f", &e, &a, &b) != 3) return 3;
            delete g;
            GpsSettings s; s.useGpsElevation = e != 0; s.gpsCovThreshold = a; s.poseCovThreshold = b;
            g = new GpsGate(s);
        } else if (!std::strcmp(cmd, "defaults")) {
            delete g;
            g = new GpsGate();
            std::printf("defaults %d %a %a\n", (int)g->S.useGpsElevation, (double)g->S.gpsCovThreshold, (double)g->S.poseCovThreshold);
        } else if (!std::strcmp(cmd, "push")) {
            GpsMessage m;
            if (std::fscanf(f, "%lf %lf %lf %lf %lf %lf %lf", &m.stamp, &m.x, &m.y, &m.z, &m.cov_x, &m.cov_y, &m.cov_z) != 7) return 3;
            g->gpsHandler(m);
        } else if (!std::strcmp(cmd, "add") || !std::strcmp(cmd, "addnokeys")) {
            const bool keys = !std::strcmp(cmd, "add");
            double t, cxx, cyy; float fr[3] = {0, 0, 0}, bk[3] = {0, 0, 0}, z;
            if (std::fscanf(f, "%lf", &t) != 1) return 3;
            if (keys && std::fscanf(f, "%f %f %f %f %f %f", fr, fr + 1, fr + 2, bk, bk + 1, bk + 2) != 6) return 3;
            if (std::fscanf(f, "%lf %lf %f", &cxx, &cyy, &z) != 3) return 3;
            GpsFactor o{};
            const bool took = g->addGPSFactor(t, keys ? fr : nullptr, keys ? bk : nullptr, cxx, cyy, z, &o);
            std::printf("%d %zu %d", (int)took, g->gpsQueue.size(), g->accepted);
            if (took) for (int k = 0; k < 3; k++) std::printf(" %a %a", (double)o.xyz[k], (double)o.variance[k]);
            std::printf("\n");
        } else {
            return 4;
        }
    }
    delete g;
    std::fclose(f);
    return 0;
}
"""

# far: front and back key poses more than 5 m apart; open: a covariance above poseCovThreshold
FAR, NEAR, EXACT = "0 0 0 6 0 0", "0 0 0 3 3.9 0", "0 0 0 3 4 0"
OPEN, SHUT, ONE = "1e8 1e8", "24.9 24.9", "3 25"


def _f(x):
    return float(np.float32(x))


# (script, expected answer lines: (took, queue left, accepted so far[, x, vx, y, vy, z, vz]))
GATE_CASES = {
    "empty queue": (f"reset 0 2 25\nadd 10 {FAR} {OPEN} 0.5", [(0, 0, 0)]),
    "no key poses": (f"reset 0 2 25\npush 10 20 0 0 0.5 0.5 0.5\naddnokeys 10 {OPEN} 0.5", [(0, 1, 0)]),
    "path below 5 m, then exactly 5 m": (f"reset 0 2 25\npush 10 20 0 0 0.5 0.5 0.5\nadd 10 {NEAR} {OPEN} 0.5\nadd 10 {EXACT} {OPEN} 0.5",
                                         [(0, 1, 0), (1, 0, 1, 20, 1, 0, 1, 0.5, 1)]),
    "covariance gate": (f"reset 0 2 25\npush 10 20 0 0 0.5 0.5 0.5\nadd 10 {FAR} {SHUT} 0.5\nadd 10 {FAR} 25 3 0.5",
                        [(0, 1, 0), (1, 0, 1, 20, 1, 0, 1, 0.5, 1)]),
    "one entry above the threshold opens the gate": (f"reset 0 2 25\npush 10 20 0 0 0.5 0.5 0.5\nadd 10 {FAR} {ONE} 0.5", [(1, 0, 1, 20, 1, 0, 1, 0.5, 1)]),
    "too old is dropped, in-window is taken": (f"reset 0 2 25\npush 9.7 50 0 0 0.5 0.5 0.5\npush 9.8 20 1 7 0.5 0.5 0.5\npush 10.1 40 0 0 0.5 0.5 0.5\n"
                                               f"add 10 {FAR} {OPEN} 0.5", [(1, 1, 1, 20, 1, 1, 1, 0.5, 1)]),
    "too new stays": (f"reset 0 2 25\npush 10.3 20 0 0 0.5 0.5 0.5\nadd 10 {FAR} {OPEN} 0.5\nadd 10.2 {FAR} {OPEN} 0.5", [(0, 1, 0), (1, 0, 1, 20, 1, 0, 1, 0.5, 1)]),
    "window edges are inside": (f"reset 0 2 25\npush 9.8 20 0 0 0.5 0.5 0.5\nadd 10 {FAR} {OPEN} 0.5\npush 10.2 40 0 0 0.5 0.5 0.5\nadd 10 {FAR} {OPEN} 0.5",
                                [(1, 0, 1, 20, 1, 0, 1, 0.5, 1), (1, 0, 2, 40, 1, 0, 1, 0.5, 1)]),
    "noisy x or y is skipped, noisy z is not": (f"reset 0 2 25\npush 10 20 0 0 2.5 0.5 0.5\npush 10 30 0 0 0.5 2.5 0.5\npush 10 40 0 0 2 2 9\nadd 10 {FAR} {OPEN} 0.5",
                                                [(1, 0, 1, 40, 2, 0, 2, 0.5, 1)]),
    "elevation off: z and its noise are replaced": (f"reset 0 2 25\npush 10 20 3 77 1.5 0.25 9\nadd 10 {FAR} {OPEN} -1.25", [(1, 0, 1, 20, 1.5, 3, 1, -1.25, 1)]),
    "elevation on": (f"reset 1 2 25\npush 10 20 3 77 1.5 0.25 9\npush 10 40 3 78 1 1 0.5\nadd 10 {FAR} {OPEN} -1.25\nadd 10 {FAR} {OPEN} -1.25",
                     [(1, 1, 1, 20, 1.5, 3, 1, 77, 9), (1, 0, 2, 40, 1, 3, 1, 78, 1)]),
    "an uninitialised fix is skipped": (f"reset 0 2 25\npush 10 1e-7 -1e-7 5 0.5 0.5 0.5\npush 10 1e-7 9 0 0.5 0.5 0.5\nadd 10 {FAR} {OPEN} 0.5",
                                        [(1, 0, 1, _f(1e-7), 1, 9, 1, 0.5, 1)]),
    "the origin quirk": (f"reset 0 2 25\npush 10 3 0 0 0.5 0.5 0.5\nadd 10 {FAR} {OPEN} 0.5\npush 10 3 4 0 0.5 0.5 0.5\nadd 10 {FAR} {OPEN} 0",
                         [(0, 0, 0), (1, 0, 1, 3, 1, 4, 1, 0, 1)]),
    "5 m spacing": (f"reset 0 2 25\npush 10 10 0 0 0.5 0.5 0.5\nadd 10 {FAR} {OPEN} 0\npush 10 12 0 0 0.5 0.5 0.5\npush 10 14.9 0 0 0.5 0.5 0.5\nadd 10 {FAR} {OPEN} 0\n"
                    f"push 10 15 0 0 0.5 0.5 0.5\nadd 10 {FAR} {OPEN} 0\npush 10 15 0 0 0.5 0.5 0.5\nadd 10 {FAR} {OPEN} 5",
                    [(1, 0, 1, 10, 1, 0, 1, 0, 1), (0, 0, 1), (1, 0, 2, 15, 1, 0, 1, 0, 1), (1, 0, 3, 15, 1, 0, 1, 5, 1)]),
    "one factor per call, the rest of the queue stays": (f"reset 0 2 25\npush 10 10 0 0 0.5 0.5 0.5\npush 10 20 0 0 0.5 0.5 0.5\npush 10.1 30 0 0 0.5 0.5 0.5\n"
                                                         f"add 10 {FAR} {OPEN} 0\nadd 10 {FAR} {SHUT} 0\nadd 10 {FAR} {OPEN} 0\nadd 10.4 {FAR} {OPEN} 0",
                                                         [(1, 2, 1, 10, 1, 0, 1, 0, 1), (0, 2, 1), (1, 1, 2, 20, 1, 0, 1, 0, 1), (0, 0, 2)]),
    "thresholds are settings": (f"reset 0 0.4 100\npush 10 20 0 0 0.5 0.3 0.5\npush 10 30 0 0 0.3 0.3 0.5\nadd 10 {FAR} 99 99 0\nadd 10 {FAR} 100 0 0",
                                [(0, 2, 0), (1, 0, 1, 30, 1, 0, 1, 0, 1)]),
}


@pytest.fixture(scope="module")
def gates(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("gps_gate")
    inc = [os.path.join(pkg.PKG_DIR, "host")]
    return {"plain": _compile(d / "plain", "gps_gate", GATE_DRIVER, inc, []), "san": _compile(d / "san", "gps_gate", GATE_DRIVER, inc, SAN)}


@pytest.mark.parametrize("which", ["plain", "san"])
def test_gps_gate_alone_takes_every_branch(gates, tmp_path, which):
    """host/lvi_gps_gate.hpp compiled alone (no HIP, no other header of the project): addGPSFactor (mapOptimization.cpp
    :1430-1507) branch by branch against answers written down here from the reference's text"""
    (tmp_path / "d.txt").write_text("defaults\n")
    out = subprocess.run([gates[which], str(tmp_path / "d.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and [float.fromhex(x) for x in out.stdout.split()[1:]] == [0.0, 2.0, 25.0]      # utility.h:178-183
    for tag, (script, want) in GATE_CASES.items():
        (tmp_path / "s.txt").write_text(script + "\n")
        out = subprocess.run([gates[which], str(tmp_path / "s.txt")], capture_output=True, text=True)
        assert out.returncode == 0, (tag, out.stdout, out.stderr)
        got = [tuple(float.fromhex(x) if "x" in x else int(x) for x in l.split()) for l in out.stdout.split("\n") if l]
        assert got == [tuple(float(np.float32(v)) if i >= 3 else v for i, v in enumerate(w)) for w in want], (tag, got)
