"""CPU tier of the pose-graph optimiser (include/lvi_pgo.h): the ABI / host-library link checks, the float64
reference tests/pgo_ref.py against central differences and known answers, the convergence condition of the GPU tier's
scenes, and csrc/lvi_pgo_math.hpp compiled alone (plain and under the host sanitizers) against the reference."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pgo_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# central differences with h = 1e-6 on errors of size <= 4: rounding 2 x 2.2e-16 x 4 / 2e-6 = 9e-10, truncation h^2 x O(1)
# = 1e-12.  The measured gap (printed by test_reference_jacobians_against_central_differences) is 4.7e-10.
H_CD, JAC_GAP_BOUND = 1e-6, 5e-9


def _declared():
    txt = open(os.path.join(ROOT, "include", "lvi_pgo.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lvi_pgo_[a-z0-9_]+)\s*\(", txt)))


# ---- ABI -------------------------------------------------------------------------------------------
def test_header_and_pgo_binding_agree(pkg):
    assert _declared() == sorted(pkg.pgo.PGO_SIGNATURES.keys())
    assert len(_declared()) == 11
    assert not set(_declared()) & set(pkg._abi.SIGNATURES), "the pgo ABI must stay out of lvi_hotpath.h's table"
    txt = open(os.path.join(ROOT, "include", "lvi_pgo.h")).read()
    assert int(re.search(r"#define LVI_PGO_MAX_POSES\s+(\d+)", txt).group(1)) == pkg.pgo.MAX_POSES == 65536
    assert int(re.search(r"#define LVI_PGO_MAX_LOOPS\s+(\d+)", txt).group(1)) == pkg.pgo.MAX_LOOPS == 64
    assert int(re.search(r"#define LVI_PGO_MAX_ITERS\s+(\d+)", txt).group(1)) == pkg.pgo.MAX_ITERS == 64
    assert int(re.search(r"#define LVI_PGO_NOT_CONVERGED\s+(\d+)", txt).group(1)) == pkg.pgo.NOT_CONVERGED == 1
    # every declaration cites the reference lines it replaces
    assert all(s in txt for s in (":1414-1428", ":1509-1527", ":1546-1566", ":1567-1599", ":1418-1420", ":1422-1427"))


def test_record_layouts(pkg):
    txt = open(os.path.join(ROOT, "include", "lvi_pgo.h")).read()
    for cname, cls, size in (("lvi_pgo_params", pkg.pgo.PgoParams, 16), ("lvi_pgo_info", pkg.pgo.PgoInfo, 32)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"\b([A-Za-z_0-9]+);", body) == [f[0] for f in cls._fields_]
        assert ctypes.sizeof(cls) == size


def test_hip_library_exports_the_pgo_abi_and_the_oracle_does_not(pkg, oracle):
    dll = ctypes.CDLL(pkg.HIP_LIB_PATH)
    for name in _declared():
        assert hasattr(dll, name), f"{name} missing from liblvi_hip.so"
    lib = pkg.pgo.bind(pkg.load_hip())
    assert lib.dll.lvi_pgo_abi_version() == 1
    assert lib.dll.lvi_abi_version() == 6
    p = pkg.pgo.PgoParams()
    lib.dll.lvi_pgo_params_default(ctypes.byref(p))
    assert (p.full_logmap, p.max_iters, p.conv_eps) == (1, R.MAX_ITERS, R.CONV_EPS)
    syms = subprocess.run(["nm", "-D", "--defined-only", oracle.path], capture_output=True, text=True).stdout
    assert "lvi_abi_version" in syms and "lvi_pgo_" not in syms


def test_pose_graph_fails_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.LviError) as e:
        pkg.PoseGraph(pkg.load_hip(), max_poses=8, max_loops=1)
    assert e.value.code == pkg._abi.LVI_ERR_NO_DEVICE


def test_host_libraries_link_with_and_without_the_pose_graph(pkg, oracle, tmp_path):
    """the oracle-linked host library builds without the pgo flattening (the node's hook is an interface of lvi_host.hpp);
    the HIP one exports it"""
    H = pkg.host_api
    out = tmp_path / "liblvi_host_oracle.so"
    H.build_host_library(str(out), os.path.dirname(oracle.path), "lvi_oracle", extra=("-fopenmp",))
    assert not H.HostLibrary(str(out)).has_pgo
    oracle_syms = subprocess.run(["nm", "-D", "--defined-only", str(out)], capture_output=True, text=True).stdout
    assert "lvh_pgo_" not in oracle_syms and "lvh_seq_use_pose_graph" not in oracle_syms
    assert os.path.exists(H.HOST_HIP_LIB), "host/liblvi_host_hip.so not built: run __graft_entry__.build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", H.HOST_HIP_LIB], capture_output=True, text=True).stdout
    for name in ("lvh_pgo_create", "lvh_pgo_destroy", "lvh_pgo_handle", "lvh_pgo_push_loop", "lvh_pgo_last", "lvh_pgo_last_error", "lvh_seq_use_pose_graph",
                 "lvh_seq_poses_corrected"):
        assert re.search(r"\b%s\b" % name, syms), name
    assert H.HostLibrary(H.HOST_HIP_LIB).has_pgo


# ---- the reference itself ------------------------------------------------------------------------------
def _cases(seed=0, count=20):
    """(Xi, Xj, Z): errors of order 1 (all branches of the closed forms) and of order 0.05 (the series)"""
    rs = np.random.RandomState(seed)
    out = []
    for trial in range(count):
        sc = 1.0 if trial < count // 2 else 0.05
        Xi = R.pose_exp(rs.normal(0, 1, 6))
        Xj = Xi @ R.pose_exp(rs.normal(0, sc, 6))
        out.append((Xi, Xj, R.pose_inv(Xi) @ Xj @ R.pose_exp(rs.normal(0, sc * 0.5, 6))))
    return out


def _central(f):
    J = np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = H_CD
        J[:, k] = (f(d) - f(-d)) / (2 * H_CD)
    return J


def jacobian_gap():
    """the largest |analytic - central difference| over the cases, both charts, prior and between factors"""
    worst = 0.0
    for full in (1, 0):
        for Xi, Xj, Z in _cases():
            r, A, B = R.between_error(Xi, Xj, Z, full)
            nA = _central(lambda d: R.between_error(Xi @ R.pose_exp(d, full), Xj, Z, full)[0])
            nB = _central(lambda d: R.between_error(Xi, Xj @ R.pose_exp(d, full), Z, full)[0])
            rp, Bp = R.prior_error(Xj, Xi @ Z, full)
            nP = _central(lambda d: R.prior_error(Xj @ R.pose_exp(d, full), Xi @ Z, full)[0])
            worst = max(worst, np.abs(A - nA).max(), np.abs(B - nB).max(), np.abs(Bp - nP).max())
    return float(worst)


def test_reference_jacobians_against_central_differences():
    gap = jacobian_gap()
    print(f"[pgo ref] analytic vs central differences (h = {H_CD}): {gap:.3e}")
    assert gap <= JAC_GAP_BOUND


def test_reference_exp_log_and_gauge():
    rs = np.random.RandomState(1)
    for full in (1, 0):
        for sc in (1.0, 0.05, 1e-5, 0.0):
            xi = rs.normal(0, 1, 6) * sc
            T = R.pose_exp(xi, full)
            assert np.abs(R.pose_log(T, full) - xi).max() < 1e-13
            assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-15
    for ang in (3.0, 3.1, 3.14, 3.1415, np.pi - 1e-9):                    # the branch near pi
        w = rs.normal(size=3)
        w *= ang / np.linalg.norm(w)
        assert np.abs(R.so3_log(R.so3_exp(w)) - w).max() < 1e-6 * (1 if ang > 3.1415 else 1e-6)
    # every between factor is blind to a common left transform: A Ad(Xi^-1) + B Ad(Xj^-1) = 0 at any linearisation point
    for full in (1, 0):
        for Xi, Xj, Z in _cases(2, 6):
            _, A, B = R.between_error(Xi, Xj, Z, full)
            assert np.abs(A @ R.adjoint(R.pose_inv(Xi)) + B @ R.adjoint(R.pose_inv(Xj))).max() < 1e-13
    p = np.array([0.3, -0.2, 2.9, 1.0, -2.0, 0.5], np.float32)
    assert np.abs(R.pose_to_rpyxyz(R.pose_from_rpyxyz(p)) - p).max() < 1e-6


def _exact_graph(full, n=12, seed=3):
    gt = [R.pose_from_rpyxyz(R.pose_to_rpyxyz(T)) for T in R.trajectory(n, seed)]
    g = R.Graph(full)
    for k in range(n):
        g.add_pose(None if k == 0 else R.pose_to_rpyxyz(gt[k - 1]), R.pose_to_rpyxyz(gt[k]))
    for frm, to in ((n - 1, 0), (2, n - 3)):
        g.add_loop(frm, to, R.pose_inv(gt[frm]) @ gt[to], 0.1)
    return g, gt


@pytest.mark.parametrize("solver", ["lstsq", "chol"])
@pytest.mark.parametrize("full", [1, 0])
def test_exact_measurements_return_ground_truth(full, solver):
    g, gt = _exact_graph(full)
    rs = np.random.RandomState(4)
    for k in range(1, len(g.X)):
        g.X[k] = g.X[k] @ R.pose_exp(np.r_[rs.normal(0, 0.02, 3), rs.normal(0, 0.1, 3)])
    info = g.solve(solver)
    assert info["converged"] and info["iterations"] <= R.MAX_ITERS - 2 and info["chi2_before"] > 1e3 and info["chi2_after"] < 1e-16
    assert max(np.abs(a - b).max() for a, b in zip(g.X, gt)) < 1e-9


@pytest.mark.parametrize("full", [1, 0])
def test_chain_without_loops_is_a_fixed_point(full):
    sc = R.scene(20, [], 11)
    for solver in ("lstsq", "chol"):
        g = R.build(sc, R.Graph(full))
        X0 = g.poses().copy()
        info = g.solve(solver)
        assert info["converged"] and info["iterations"] == 1 and info["max_step"] < 1e-12 and info["chi2_after"] < 1e-20
        assert np.abs(g.poses() - X0).max() < 1e-12


def test_add_loop_refuses_what_the_library_refuses():
    g = R.build(R.scene(5, [], 1), R.Graph())
    for frm, to, var in ((2, 2, 0.1), (-1, 2, 0.1), (2, 5, 0.1), (1, 2, 0.0), (1, 2, -1.0)):
        with pytest.raises(ValueError):
            g.add_loop(frm, to, np.eye(4), var)


# ---- the GPU tier's scenes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.GPU_SCENES))
def test_gpu_scenes_converge_within_the_margin(name):
    """every scene of tests/test_gpu_pgo.py, both charts, both linear solvers: converged within max_iters - 2 steps — the
    condition that lets the device use an undamped solver — and the loop error within what the odometry drift allows"""
    n, loops, _, _ = R.GPU_SCENES[name]
    sc = R.gpu_scene(name)
    assert len(sc["poses"]) == n and len(sc["loops"]) == len(loops)
    X0 = [R.pose_from_rpyxyz(p) for p in sc["poses"]]
    for frm, to, Z, var in sc["loops"]:
        E = R.pose_inv(Z) @ R.pose_inv(X0[frm]) @ X0[to]
        assert R.rot_angle(E[:3, :3]) < np.deg2rad(5.0) and np.linalg.norm(E[:3, 3]) < 0.5 and 0.05 <= var <= 0.3
    for full in (1, 0):
        (Xa, ia), (Xb, ib) = R.solve_both(R.build(sc, R.Graph(full)))
        (gr, gt), (g0r, g0t) = R.gaps(Xa, Xb)
        print(f"[pgo ref] {name} full_logmap {full}: iterations {ia['iterations']} / {ib['iterations']}, steps {['%.1e' % s for s in ia['steps']]}, "
              f"G relative ({gr:.3e}, {gt:.3e}), G key 0 ({g0r:.3e}, {g0t:.3e})")
        for info in (ia, ib):
            assert info["converged"] and info["iterations"] <= R.MAX_ITERS - 2, (name, full, info["steps"])
        assert max(gr, gt, g0r, g0t) < 10 * R.CONV_EPS


def test_gpu_scene_shapes():
    S = R.GPU_SCENES
    assert [S[k][0] for k in ("n1", "n2", "n3_loop", "n37", "n300", "n1025")] == [1, 2, 3, 37, 300, 1025]
    assert S["n3_loop"][1] == [(2, 0)] and len(S["n37"][1]) == 3 and len(S["n300"][1]) == 5 and len(S["n1025"][1]) == 8
    l37 = S["n37"][1]
    nodes = [x for ft in l37 for x in ft]
    assert any(nodes.count(x) == 2 for x in nodes)                       # two loops share a node
    assert any(f == t + 1 for f, t in l37) and any(f < t for f, t in l37)
    yaw = R.gpu_scene("yaw_pi")["poses"][:, 2]
    assert np.abs(np.diff(yaw)).max() > 6.0 and yaw.max() > 3.0 and yaw.min() < -3.0     # the heading wraps through +-pi


def test_full_system_stalls_in_the_gauge_and_agrees_relative_to_key_0():
    """the finding behind the anchored step (pgo_ref's docstring): solved as it stands, the system never reaches
    max|delta| < 1e-10 with either linear solver — the stall is a common translation — while the poses relative to key 0
    are the anchored answer"""
    sc = R.gpu_scene("n37")
    g = R.build(sc, R.Graph(1))
    info = g.solve("lstsq")
    for solver in ("lstsq", "chol"):
        f = R.build(sc, R.Graph(1))
        fi = f.solve(solver, gauge="full")
        (dr, dt), (d0r, d0t) = R.gaps(g.poses(), f.poses())
        print(f"[pgo ref] full system, {solver}: steps {['%.1e' % s for s in fi['steps']]}; vs anchored: relative ({dr:.3e}, {dt:.3e}), key 0 ({d0r:.3e}, {d0t:.3e})")
        assert not fi["converged"] and fi["iterations"] == R.MAX_ITERS and min(fi["steps"]) > R.CONV_EPS
        assert dr < 10 * R.CONV_EPS and dt < 10 * R.CONV_EPS and d0r < 10 * R.CONV_EPS
    assert info["converged"]


# ---- csrc/lvi_pgo_math.hpp alone, under the host sanitizers ------------------------------------------------
DRIVER = r"""
// stand-alone driver of csrc/lvi_pgo_math.hpp: the SE(3) pieces the kernels call, run on the host
#include <cstdio>
#include <cstring>
#include <vector>
#include "lvi_pgo_math.hpp"
using namespace lvi_pgo_math;

static void put(const double* v, int n) { for (int i = 0; i < n; i++) std::printf(" %a", v[i]); }

int main(int argc, char** argv)
{
    if (argc < 3) return 1;
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    if (!std::strcmp(argv[1], "edges")) {
        // records: int32 full, then Xi, Xj, Z as 4x4 doubles
        int32_t full;
        while (std::fread(&full, 4, 1, f) == 1) {
            double M[48];
            if (std::fread(M, 8, 48, f) != 48) return 3;
            Pose Xi, Xj, Z, ZX;
            pose_from_matrix(M, &Xi); pose_from_matrix(M + 16, &Xj); pose_from_matrix(M + 32, &Z);
            double r[6], A[36], B[36], rp[6], Bp[36];
            between_error(Xi, Xj, Z, full, r, A, B);
            pose_mul(Xi, Z, &ZX);
            prior_error(Xj, ZX, full, rp, Bp);
            put(r, 6); put(A, 36); put(B, 36); put(rp, 6); put(Bp, 36);
            // a whitened normal block and its two solvers
            double Hm[36], L[36], x[6], y[6], Bc[36];
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < 6; j++) { Hm[6 * i + j] = i == j ? 1e-3 : 0.; for (int k = 0; k < 6; k++) Hm[6 * i + j] += B[6 * k + i] * B[6 * k + j]; }
            for (int i = 0; i < 6; i++) { x[i] = r[i]; y[i] = r[i]; }
            chol6(Hm, L);
            chol6_solve(L, x);
            std::memcpy(Bc, Hm, sizeof(Bc));
            solve6(Bc, y);
            put(Hm, 36); put(x, 6); put(y, 6);
            std::printf("\n");
        }
    } else if (!std::strcmp(argv[1], "expmap")) {
        // records: int32 full, xi [6] -> Expmap (4x4), Logmap of it, X * Retract(xi) for X = Expmap
        int32_t full;
        while (std::fread(&full, 4, 1, f) == 1) {
            double xi[6], M[16], back[6];
            if (std::fread(xi, 8, 6, f) != 6) return 3;
            Pose T;
            pose_exp(xi, full, &T);
            pose_to_matrix(T, M);
            pose_log(T, full, back);
            put(M, 16); put(back, 6);
            pose_retract(&T, xi, full);
            pose_to_matrix(T, M);
            put(M, 16);
            std::printf("\n");
        }
    } else if (!std::strcmp(argv[1], "rpy")) {
        // records: float pose [6] -> the 4x4 and the float pose read back
        float p[6];
        while (std::fread(p, 4, 6, f) == 6) {
            Pose T;
            double M[16];
            float q[6];
            pose_from_rpyxyz(p, &T);
            pose_to_matrix(T, M);
            pose_to_rpyxyz(T, q);
            put(M, 16);
            for (int i = 0; i < 6; i++) std::printf(" %a", (double)q[i]);
            std::printf("\n");
        }
    } else {
        return 1;
    }
    std::fclose(f);
    return 0;
}
"""


def _build_driver(pkg, d, flags):
    d.mkdir(exist_ok=True)
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", *flags, "-I" + os.path.join(pkg.PKG_DIR, "csrc"), "-o", str(exe),
                        str(d / "driver.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.fixture(scope="module")
def drivers(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("pgo_header")
    return {"plain": _build_driver(pkg, d / "plain", []),
            "san": _build_driver(pkg, d / "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])}


@pytest.fixture(scope="module")
def header_tol():
    """a small multiple (4 x) of the reference's own analytic-versus-central-difference gap, measured in this tier"""
    return 4.0 * jacobian_gap()


def _run(exe, mode, path):
    r = subprocess.run([exe, mode, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return [np.array([float.fromhex(x) for x in l.split()]) for l in r.stdout.split("\n") if l]


@pytest.mark.parametrize("which", ["plain", "san"])
def test_math_header_errors_and_jacobians_equal_the_reference(drivers, header_tol, tmp_path, which):
    blob, want = b"", []
    for full in (1, 0):
        for Xi, Xj, Z in _cases():
            blob += struct.pack("<i", full) + np.array([Xi, Xj, Z], np.float64).tobytes()
            r, A, B = R.between_error(Xi, Xj, Z, full)
            rp, Bp = R.prior_error(Xj, Xi @ Z, full)
            Hm = B.T @ B + 1e-3 * np.eye(6)
            want.append(np.r_[r, A.ravel(), B.ravel(), rp, Bp.ravel(), Hm.ravel(), np.linalg.solve(Hm, r), np.linalg.solve(Hm, r)])
    (tmp_path / "e.bin").write_bytes(blob)
    got = _run(drivers[which], "edges", tmp_path / "e.bin")
    assert len(got) == len(want) == 40
    worst = max(np.abs(g[:120] - w[:120]).max() for g, w in zip(got, want))
    worst_solve = max((np.abs(g[120:] - w[120:]) / np.maximum(1.0, np.abs(w[120:]))).max() for g, w in zip(got, want))
    print(f"[pgo header] {which}: errors and Jacobians vs reference {worst:.3e} (tolerance {header_tol:.3e}); 6x6 solves {worst_solve:.3e}")
    assert 0 < header_tol < 4 * JAC_GAP_BOUND and worst <= header_tol
    assert worst_solve <= 1e-9                                            # cond(B'B + 1e-3 I) <= 1e6 here


@pytest.mark.parametrize("which", ["plain", "san"])
def test_math_header_expmap_logmap_and_rpy_equal_the_reference(drivers, header_tol, tmp_path, which):
    rs = np.random.RandomState(5)
    blob, want = b"", []
    for full in (1, 0):
        for sc in (1.0, 1.0, 2.5, 0.19, 0.21, 0.05, 1e-4, 1e-9, 0.0):   # both sides of the series switch (theta^2 = 0.04)
            xi = rs.normal(0, 1, 6)
            xi *= sc / max(np.linalg.norm(xi[:3]), 1e-300) if sc else 0.0
            blob += struct.pack("<i", full) + xi.tobytes()
            T = R.pose_exp(xi, full)
            want.append(np.r_[T.ravel(), R.pose_log(T, full), (T @ R.pose_exp(xi, full)).ravel()])
    (tmp_path / "x.bin").write_bytes(blob)
    got = _run(drivers[which], "expmap", tmp_path / "x.bin")
    assert len(got) == len(want)
    worst = max(np.abs(g - w).max() for g, w in zip(got, want))
    print(f"[pgo header] {which}: Expmap / Logmap / retract vs reference {worst:.3e}")
    assert worst <= header_tol
    poses = np.array([[0.3, -0.2, 2.9, 1.0, -2.0, 0.5], [0, 0, 0, 0, 0, 0], [-0.05, 0.04, -3.1, 80.0, -75.5, 0.3], [0.01, 1.2, 3.14159, -4.0, 2.0, 9.0]], np.float32)
    (tmp_path / "p.bin").write_bytes(poses.tobytes())
    got = _run(drivers[which], "rpy", tmp_path / "p.bin")
    for g, p in zip(got, poses):
        T = R.pose_from_rpyxyz(p)
        assert np.abs(g[:16] - T.ravel()).max() <= 1e-15 * 80
        # the float casts: equal unless the double sits on a rounding boundary, where one float ulp may separate two libms
        assert np.abs(g[16:] - R.pose_to_rpyxyz(T).astype(np.float64)).max() <= 2.0 ** -23 * max(1.0, float(np.abs(p).max()))
