"""CPU tier of the device PnP RANSAC (include/lvi_pnp.h): known answers of the host restatement
tests/pnp_ref.py on synthetic scenes, the input condition of the GPU tier's list, the host-only headers under the host
sanitizers, and the ABI / host-library link checks."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pnp_ref as P
from fmat_ref import update_num_iters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "lvi_pnp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lvi_pnp_[a-z0-9_]+)\s*\(", txt)))


# ---- ABI -------------------------------------------------------------------------------------------
def test_header_and_pnp_binding_agree(pkg):
    assert _declared() == sorted(pkg.pnp.PNP_SIGNATURES.keys())
    assert len(_declared()) == 5
    assert not set(_declared()) & set(pkg._abi.SIGNATURES), "the pnp ABI must stay out of lvi_hotpath.h's table"
    txt = open(os.path.join(ROOT, "include", "lvi_pnp.h")).read()
    assert int(re.search(r"#define LVI_PNP_MAX_POINTS\s+(\d+)", txt).group(1)) == pkg.pnp.MAX_POINTS == 2048
    assert int(re.search(r"#define LVI_PNP_MAX_ITERS\s+(\d+)", txt).group(1)) == pkg.pnp.MAX_ITERS == 1024


def test_info_record_layout(pkg):
    txt = open(os.path.join(ROOT, "include", "lvi_pnp.h")).read()
    body = re.search(r"typedef struct lvi_pnp_info \{(.*?)\} lvi_pnp_info;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b([A-Za-z_]+)(?:\[\d+\])?;", body)
    assert names == [f[0] for f in pkg.pnp.PnPInfo._fields_]
    assert ctypes.sizeof(pkg.pnp.PnPInfo) == 6 * 4 + 9 * 8 + 3 * 8 + 8


def test_hip_library_exports_the_pnp_abi_and_the_oracle_does_not(pkg, oracle):
    dll = ctypes.CDLL(pkg.HIP_LIB_PATH)
    for name in _declared():
        assert hasattr(dll, name), f"{name} missing from liblvi_hip.so"
    lib = pkg.pnp.bind(pkg.load_hip())
    assert lib.dll.lvi_pnp_abi_version() == 1
    assert lib.dll.lvi_abi_version() == 6
    syms = subprocess.run(["nm", "-D", "--defined-only", oracle.path], capture_output=True, text=True).stdout
    assert "lvi_abi_version" in syms and "lvi_pnp_" not in syms


def test_pnp_ransac_fails_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.LviError) as e:
        pkg.PnPRansac(pkg.load_hip())
    assert e.value.code == pkg._abi.LVI_ERR_NO_DEVICE


def test_host_libraries_link_with_and_without_the_loop_confirmation(pkg, oracle, tmp_path):
    """the oracle-linked host library builds without the pnp flattening; the HIP one exports it"""
    H = pkg.host_api
    out = tmp_path / "liblvi_host_oracle.so"
    H.build_host_library(str(out), os.path.dirname(oracle.path), "lvi_oracle", extra=("-fopenmp",))
    assert not H.HostLibrary(str(out)).has_pnp
    oracle_syms = subprocess.run(["nm", "-D", "--defined-only", str(out)], capture_output=True, text=True).stdout
    assert "lvh_pnp_" not in oracle_syms and "lvh_bow_use_pnp" not in oracle_syms
    assert os.path.exists(H.HOST_HIP_LIB), "host/liblvi_host_hip.so not built: run __graft_entry__.build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", H.HOST_HIP_LIB], capture_output=True, text=True).stdout
    for name in ("lvh_pnp_create", "lvh_pnp_destroy", "lvh_pnp_handle", "lvh_pnp_status", "lvh_pnp_last_error", "lvh_bow_use_pnp", "lvh_bow_pnp_connection"):
        assert re.search(r"\b%s\b" % name, syms), name
    assert H.HostLibrary(H.HOST_HIP_LIB).has_pnp


# ---- the sample stream and RANSACUpdateNumIters ---------------------------------------------------------
def _recurrence(count):
    s, out = 0xFFFFFFFFFFFFFFFF, []
    for _ in range(count):
        s = ((s & 0xFFFFFFFF) * 4164903690 + (s >> 32)) % (1 << 64)
        out.append(s % (1 << 32))
    return out


@pytest.mark.parametrize("n", [6, 7, 26, 150])
def test_sample_stream_matches_the_recurrence_written_out(n):
    """5 distinct indices per subset; a draw that repeats an earlier index of the same subset is redrawn"""
    raw = iter(_recurrence(4000))
    want, redraws = [], 0
    for _ in range(100):
        idx = []
        while len(idx) < 5:
            k = next(raw) % n
            if k in idx:
                redraws += 1
                continue
            idx.append(k)
        want.append(idx)
    got = P.sample_stream(n, 100)
    assert got == want
    assert all(len(set(s)) == 5 and 0 <= min(s) and max(s) < n for s in got)
    if n <= 7:
        assert redraws > 50                                              # the redraw path is exercised
    assert P.sample_stream(5, 100) == [[0, 1, 2, 3, 4]]


def test_update_num_iters_hand_values():
    assert update_num_iters(0.99, 0.0, 5, 100) == 0                    # 1 - 1^5 = 0 < DBL_MIN: stop after this iteration
    assert update_num_iters(0.99, 0.5, 5, 100) == 100                  # log(0.01) / log(1 - 0.5^5) = 145.05 >= 100
    assert update_num_iters(0.99, 0.2, 5, 100) == 12                   # -4.60517 / log(0.67232) = 11.6
    assert abs(np.log(0.01) / np.log(1 - 0.5 ** 5) - 145.05) < 0.01 and abs(np.log(0.01) / np.log(1 - 0.8 ** 5) - 11.6) < 0.01


def test_threshold_is_the_float_parameter_squared():
    thr = np.float32(10.0 / 460.0)
    assert P.THRESHOLD == float(thr) and P.threshold_f32(P.THRESHOLD) == np.float32(float(thr) * float(thr))
    assert P.threshold_f32(10.0 / 460.0) == P.threshold_f32(P.THRESHOLD)    # the double is rounded to float first


# ---- EPnP ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 50])
def test_epnp_recovers_the_pose_of_exact_points(n):
    """bounds measured with eig="lapack" over seeds 0..19 (pnp_ref.EXACT_*: rep 1.8e-8, |dR| 1.1e-7, |dt| 1.1e-6, all
    f32 rounding of the inputs seen through the geometry); asserted at 10 x on the code under test"""
    for seed in range(20):
        p3, p2, _, (R, t) = P.scene(n, seed=seed)
        m = P.epnp(p3, p2)
        assert m is not None and m["which_beta"] in (1, 2, 3)
        assert m["rep"] <= 10 * P.EXACT_REP, (seed, m["rep"])
        assert np.abs(m["R"] - R).max() <= 10 * P.EXACT_DR and np.abs(m["t"] - t).max() <= 10 * P.EXACT_DT, seed
        assert abs(np.linalg.det(m["R"]) - 1) < 1e-12 and np.abs(m["R"] @ m["R"].T - np.eye(3)).max() < 1e-12


def test_jacobi_against_lapack():
    """eigenvalues of M'M to 1e-13 of the largest; the null space span(v[0], v[1]) of a 5-point M'M as a projector"""
    worst_res = 0.0
    for n, seed in ((5, 0), (5, 1), (5, 2), (50, 3), (50, 4)):
        p3, p2, _, _ = P.scene(n, 0.0, 1.0 / P.FOCAL_LENGTH, seed)
        m = P.epnp(p3, p2, detail=True)
        S = m["S"]
        lam, V, res = P.eig12_jacobi(S, residue=True)
        worst_res = max(worst_res, res)
        w, E = np.linalg.eigh(S)
        assert np.abs(np.sort(lam) - w).max() <= 1e-13 * np.abs(w).max()
        assert np.abs(V.T @ V - np.eye(12)).max() < 1e-14
        idx = P.smallest4([float(x) for x in lam])
        assert [float(lam[i]) for i in idx] == sorted(float(x) for x in lam)[:4]
        if n == 5:
            assert w[1] < 1e-12 * w[-1] < w[2]                            # ten rows: a two-dimensional null space
            Pj = V[:, idx[:2]] @ V[:, idx[:2]].T
            Pl = E[:, :2] @ E[:, :2].T
            assert np.abs(Pj - Pl).max() < 1e-10
    assert worst_res < 1e-15                                              # off-diagonal Frobenius norm / largest eigenvalue after SWEEPS12 sweeps
    assert P.smallest4([3.0, 1.0, 2.0, 1.0] + [9.0] * 8) == [3, 1, 2, 0]    # among equals the higher index first


def test_decompositions_on_known_matrices():
    lam, E = P.eig3_jacobi([[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 5.0]])
    assert np.allclose(lam, [5.0, 3.0, 1.0], atol=1e-15)
    assert np.allclose(np.abs(np.array(E)[:, 0]), [0, 0, 1]) and np.allclose(np.abs(np.array(E)[:, 2]), [2 ** -0.5, 2 ** -0.5, 0])
    assert P.inv3([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [1.0, 0.0, 1.0]]) is None            # an exactly zero pivot
    assert np.allclose(P.inv3([[0.0, 2.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 4.0]]), [[0, 1, 0], [0.5, 0, 0], [0, 0, 0.25]])
    rs = np.random.RandomState(0)
    A, b = rs.normal(size=(6, 4)), rs.normal(size=6)
    assert np.allclose(P.lstsq(A.tolist(), b.tolist()), np.linalg.lstsq(A, b, rcond=None)[0], atol=1e-13)
    assert P.lstsq([[0.0] * 3] * 6, [1.0] * 6) == [0.0] * 3
    B = rs.normal(size=(3, 3))
    U, _, Vt = np.linalg.svd(B)
    assert np.allclose(P.polar3_jacobi(B.tolist()), U @ Vt, atol=1e-13)


# ---- RANSAC -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outliers", [0.2, 0.4])
def test_planted_outliers_are_rejected(outliers):
    for seed in range(3):
        for noise in (0.0, 0.5 / P.FOCAL_LENGTH, 2.0 / P.FOCAL_LENGTH):
            p3, p2, truth, _ = P.scene(150, outliers, noise, 500 + seed)
            st, T = P.solve(p3, p2)
            # a planted outlier is uniform in +-0.8; none of these seeds lands one within 10/460 of its point's projection
            assert T["best_iter"] >= 0 and not st[~truth].any(), (seed, noise)
            assert st[truth].mean() >= 0.9, (seed, noise, st[truth].mean())
            if noise == 0:
                assert st[truth].all() and not st[~truth].any()


def test_singular_control_points_give_no_model_and_the_walk_continues():
    p3, p2, truth, _ = P.scene(30, 0.0, 0.0, 9)
    first = P.sample_stream(30, 100)[0]
    p3 = p3.copy()
    p3[first, 2] = 8.0                                                   # the first subset exactly coplanar (z - mean z == 0 exactly)
    assert P.epnp(p3[first], p2[first]) is None
    st, T = P.solve(p3, p2)
    assert not T["has_model"][0] and T["models"][0] is None and T["good"][0] == 0
    assert T["best_iter"] >= 1 and T["iters"] > 1 and st.sum() >= 25   # the five moved points no longer fit


def test_status_edge_cases():
    p3, p2, _, _ = P.scene(5, seed=2)
    st, T = P.solve(p3, p2)
    assert T["path"] == "direct" and st.tolist() == [1] * 5 and T["iters"] == 1 and T["n_subsets"] == 1
    p3b = p3.copy()
    p3b[:, 2] = 8.0
    st, T = P.solve(p3b, p2)                                             # n == 5 and no model: all zeros
    assert st.tolist() == [0] * 5 and T["best_iter"] == -1
    for n in (0, 4):
        with pytest.raises(ValueError):
            P.solve(p3[:n], p2[:n])
    # nothing acceptable: random image points, no hypothesis collects more than four inliers
    rs = np.random.RandomState(3)
    q3, q2, _, _ = P.scene(40, seed=4)
    q2 = rs.uniform(-0.8, 0.8, q2.shape).astype(np.float32)
    st, T = P.solve(q3, q2)
    assert T["best_iter"] == -1 and T["iters"] == 100 and not st.any() and not T["R"].any()
    assert P.walk(40, 100, [True] * 100, [4] * 100) == (100, -1) and P.walk(40, 100, [False] + [True] * 99, [40] * 100) == (2, 1)


# ---- the host-only headers under the host sanitizers ----------------------------------------------------------
DRIVER = r"""
// stand-alone driver of the host-only headers of include/lvi_pnp.h: the sample stream and the EPnP arithmetic
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "lvi_ransac.hpp"
#include "lvi_pnp_math.hpp"
using namespace lvi_pnp_math;

static int epnp_host(const std::vector<double>& pw, const std::vector<double>& uv, int n, double* R, double* t)
{
    std::vector<double> al(4 * n), M(24 * n), pcs(3 * n);
    double cws[12];
    if (!pnp_control_points(pw.data(), n, cws, al.data())) return 0;
    pnp_fill_m(al.data(), uv.data(), n, M.data());
    double A[144], V[144], B[144], W[144], cs[12];
    for (int i = 0; i < 12; i++)
        for (int j = 0; j < 12; j++) { A[12 * i + j] = pnp_mtm(M.data(), 2 * n, i, j); V[12 * i + j] = i == j ? 1. : 0.; }
    for (int sw = 0; sw < PNP_SWEEPS12; sw++)
        for (int r = 0; r < 11; r++) {
            for (int k = 0; k < 6; k++) {
                int p, q;
                jacobi12_pair(r, k, &p, &q);
                pnp_rot(A[12 * p + q], A[12 * p + p], A[12 * q + q], &cs[2 * k], &cs[2 * k + 1]);
            }
            for (int e = 0; e < 144; e++) B[e] = jacobi12_row(A, 12, cs, r, e / 12, e % 12);
            for (int e = 0; e < 144; e++) { A[e] = jacobi12_col(B, 12, cs, r, e / 12, e % 12); W[e] = jacobi12_col(V, 12, cs, r, e / 12, e % 12); }
            std::memcpy(V, W, sizeof(V));
        }
    double lam[12], v4[48], L[60], rho[6], rep[4] = {0, 0, 0, 0}, Rs[3][9], ts[3][3];
    int idx[4];
    for (int i = 0; i < 12; i++) lam[i] = A[13 * i];
    pnp_smallest4(lam, idx);
    for (int k = 0; k < 4; k++)
        for (int j = 0; j < 12; j++) v4[12 * k + j] = V[12 * j + idx[k]];
    pnp_l_rho(v4, cws, L, rho);
    for (int N = 1; N <= 3; N++) rep[N] = pnp_candidate(N, L, rho, v4, al.data(), pw.data(), uv.data(), n, pcs.data(), Rs[N - 1], ts[N - 1]);
    const int N = pnp_choose(rep);
    std::memcpy(R, Rs[N - 1], sizeof(double) * 9);
    std::memcpy(t, ts[N - 1], sizeof(double) * 3);
    return N;
}

int main(int argc, char** argv)
{
    if (argc >= 4 && !std::strcmp(argv[1], "stream")) {
        const int n = std::atoi(argv[2]), count = std::atoi(argv[3]);
        std::vector<int32_t> sub(5 * (size_t)(count > 0 ? count : 0) + 5);
        const int got = lvi_ransac::sample_stream<5>(n, count, 1, [](const int32_t*) { return true; }, sub.data());   // as lvi_pnp_solve calls it
        for (int h = 0; h < got; h++) std::printf("%d %d %d %d %d\n", sub[5 * h], sub[5 * h + 1], sub[5 * h + 2], sub[5 * h + 3], sub[5 * h + 4]);
        if (n >= 5) for (int g = 0; g <= n; g++) std::printf("log %a\n", lvi_ransac::update_log<5>(n, g));
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "epnp")) {
        // file: int32 n, then n x (x y z u v) float, repeated
        FILE* f = std::fopen(argv[2], "rb");
        if (!f) return 2;
        int32_t n;
        while (std::fread(&n, 4, 1, f) == 1 && n > 0) {
            std::vector<float> raw(5 * (size_t)n);
            if (std::fread(raw.data(), 4, raw.size(), f) != raw.size()) return 3;
            std::vector<double> pw(3 * n), uv(2 * n);
            for (int i = 0; i < n; i++) { for (int j = 0; j < 3; j++) pw[3 * i + j] = raw[5 * i + j]; for (int j = 0; j < 2; j++) uv[2 * i + j] = raw[5 * i + 3 + j]; }
            double R[9] = {0}, t[3] = {0};
            const int N = epnp_host(pw, uv, n, R, t);
            std::printf("model %d", N);
            for (int k = 0; k < 9; k++) std::printf(" %a", R[k]);
            for (int k = 0; k < 3; k++) std::printf(" %a", t[k]);
            int good = 0;
            for (int i = 0; i < n; i++) good += pnp_error(R, t, raw[5 * i], raw[5 * i + 1], raw[5 * i + 2], raw[5 * i + 3], raw[5 * i + 4]) <= (float)1e-4;
            std::printf(" %d\n", good);
        }
        std::fclose(f);
        return 0;
    }
    return 1;
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
    d = tmp_path_factory.mktemp("pnp_headers")
    return {"plain": _build_driver(pkg, d / "plain", []),
            "san": _build_driver(pkg, d / "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])}


@pytest.mark.parametrize("which", ["plain", "san"])
def test_stream_header_equals_the_restatement(drivers, which):
    """csrc/lvi_ransac.hpp with modelPoints = 5: the subsets and the log table the device walk reads"""
    for n, count in ((5, 3), (6, 100), (26, 100), (150, 100), (2048, 1024), (4, 10)):
        r = subprocess.run([drivers[which], "stream", str(n), str(count)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [l for l in r.stdout.split("\n") if l]
        subs = [list(map(int, l.split())) for l in lines if not l.startswith("log")]
        logs = [float.fromhex(l.split()[1]) for l in lines if l.startswith("log")]
        if n < 5:
            assert not subs and not logs
            continue
        rng = P.CvRng()
        assert subs == [P.get_subset(rng, n) for _ in range(count)]
        assert len(logs) == n + 1 and logs[n] == float("inf")            # ep = 0: denom < DBL_MIN
        for g in (0, 1, n // 2, n - 1):
            # update_num_iters(p, ep, 5, N) == N unless num / denom < N: recompute from the table as the device does
            num = np.log(max(1.0 - 0.99, 2.2250738585072014e-308))
            want = update_num_iters(0.99, (n - g) / n, 5, 100)
            got = 100 if logs[g] >= 0 or -num >= 100 * -logs[g] else int(round(num / logs[g]))
            assert got == want, (n, g)


@pytest.mark.parametrize("which", ["plain", "san"])
def test_math_header_equals_the_restatement_bit_for_bit(drivers, tmp_path, which):
    """csrc/lvi_pnp_math.hpp run on the host (the functions the kernel calls, the Jacobi entries visited in a loop):
    which_beta, R and t of pnp_ref.epnp to the last bit, and the no-model answer"""
    blob, want = b"", []
    for n, o, noise, seed in [(5, 0, 0, 1), (5, 0, 2 / 460, 2), (5, 0.2, 0.5 / 460, 3), (50, 0, 0, 4), (50, 0.2, 2 / 460, 5), (7, 0, 1 / 460, 6), (5, 0, 0, 7)]:
        p3, p2, _, _ = P.scene(n, o, noise, seed)
        if seed == 7:
            p3[:, 2] = 8.0
        blob += struct.pack("<i", n) + np.c_[p3, p2].astype(np.float32).tobytes()
        want.append(P.epnp(p3, p2))
    (tmp_path / "e.bin").write_bytes(blob)
    r = subprocess.run([drivers[which], "epnp", str(tmp_path / "e.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.split("\n") if l]
    assert len(lines) == len(want) and want[-1] is None
    for tok, w in zip(lines, want):
        if w is None:
            assert tok[1] == "0"
            continue
        got = np.array([float.fromhex(x) for x in tok[2:14]])
        assert int(tok[1]) == w["which_beta"]
        assert got.tobytes() == np.r_[w["R"].ravel(), w["t"]].tobytes()


# ---- the GPU tier's list ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", P.GPU_NS)
def test_gpu_list_is_not_rounding_decided(n):
    """status, inlier count and iteration count of every call of tests/test_gpu_pnp.py's list are the same with this
    restatement's Jacobi decompositions and with LAPACK's: no call's answer hangs on a rounding.  A cell that fails is
    taken out of the list in pnp_ref.GPU_REMOVED (two were), never skipped here."""
    cases = [c for c in P.gpu_cases() if c[0] == n]
    assert len(cases) >= (6 if n == 5 else 16)
    for _, o, noise, seed in cases:
        p3, p2, _, _ = P.scene(n, o, noise, seed)
        a, Ta = P.solve(p3, p2, eig="jacobi")
        b, Tb = P.solve(p3, p2, eig="lapack")
        assert (a == b).all() and Ta["n_inliers"] == Tb["n_inliers"] and Ta["iters"] == Tb["iters"], (n, o, noise, seed)


def test_gpu_list_shape():
    cases = P.gpu_cases()
    assert len(cases) == 142 and len({c[3] for c in cases}) == len(cases)
    assert {c[0] for c in cases} == set(P.GPU_NS) and max(c[1] for c in cases) == 0.4
    assert len(cases) == 8 * 3 * 3 * 2 - len(P.GPU_REMOVED)             # floor(0.2 * 5) = 1: no cell is without its outlier
