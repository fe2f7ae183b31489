"""CPU tier of the device RANSAC (include/lvi_fmat.h): known answers of the host restatement tests/fmat_ref.py
on synthetic two-view geometry, and the ABI / host-library link checks."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fmat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "lvi_fmat.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lvi_fmat_[a-z0-9_]+)\s*\(", txt)))


# ---- ABI -------------------------------------------------------------------------------------------
def test_header_and_fmat_binding_agree(pkg):
    assert _declared() == sorted(pkg.fmat.FMAT_SIGNATURES.keys())
    assert not set(_declared()) & set(pkg._abi.SIGNATURES), "the fmat ABI must stay out of lvi_hotpath.h's table"


def test_info_record_layout(pkg):
    txt = open(os.path.join(ROOT, "include", "lvi_fmat.h")).read()
    body = re.search(r"typedef struct lvi_fmat_info \{(.*?)\} lvi_fmat_info;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b([A-Za-z_]+)(?:\[\d+\])?;", body)
    assert names == [f[0] for f in pkg.fmat.FmatInfo._fields_]
    assert ctypes.sizeof(pkg.fmat.FmatInfo) == 6 * 4 + 8 + 9 * 8 + 8


def test_hip_library_exports_the_fmat_abi(pkg):
    dll = ctypes.CDLL(pkg.HIP_LIB_PATH)
    for name in _declared():
        assert hasattr(dll, name), f"{name} missing from liblvi_hip.so"
    lib = pkg.fmat.bind(pkg.load_hip())
    assert lib.dll.lvi_fmat_abi_version() == 1
    assert lib.dll.lvi_abi_version() == 6


def test_fundamental_ransac_fails_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.LviError) as e:
        pkg.FundamentalRansac(pkg.load_hip())
    assert e.value.code == pkg._abi.LVI_ERR_NO_DEVICE


def test_host_libraries_link_with_and_without_the_device_ransac(pkg, oracle, tmp_path):
    """the oracle-linked host library builds without the fmat flattening; the HIP one exports it"""
    H = pkg.host_api
    out = tmp_path / "liblvi_host_oracle.so"
    H.build_host_library(str(out), os.path.dirname(oracle.path), "lvi_oracle", extra=("-fopenmp",))
    hl = H.HostLibrary(str(out))
    assert not hl.has_fmat
    oracle_syms = subprocess.run(["nm", "-D", "--defined-only", str(out)], capture_output=True, text=True).stdout
    assert "lvh_trk_use_device_fundamental" not in oracle_syms
    assert os.path.exists(H.HOST_HIP_LIB), "host/liblvi_host_hip.so not built: run __graft_entry__.build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", H.HOST_HIP_LIB], capture_output=True, text=True).stdout
    assert "lvh_trk_use_device_fundamental" in syms
    assert H.HostLibrary(H.HOST_HIP_LIB).has_fmat


# ---- cv::RNG and RANSACUpdateNumIters ---------------------------------------------------------------
def test_rng_matches_the_recurrence_written_out():
    # state_{k+1} = lo32(state_k) * 4164903690 + hi32(state_k), output lo32; seed 2^64 - 1
    s = 0xFFFFFFFFFFFFFFFF
    want = []
    for _ in range(6):
        s = ((s & 0xFFFFFFFF) * 4164903690 + (s >> 32)) % (1 << 64)
        want.append(s % (1 << 32))
    rng = R.CvRng()
    assert [rng.next() for _ in range(6)] == want
    # the first value by hand: 0xFFFFFFFF * 4164903690 + 0xFFFFFFFF = 4164903691 * (2^32 - 1)
    assert want[0] == (4164903691 * 0xFFFFFFFF) % (1 << 32)
    rng = R.CvRng()
    assert [rng.uniform(0, 150) for _ in range(4)] == [w % 150 for w in want[:4]]


def test_update_num_iters_hand_values():
    assert R.update_num_iters(0.99, 0.0, 7, 1000) == 0              # 1 - 1^7 = 0 < DBL_MIN: stop after this iteration
    assert R.update_num_iters(0.99, 0.5, 7, 1000) == 587            # 4.6052 / 0.0078431 = 587.16
    assert R.update_num_iters(0.99, 0.45, 7, 1000) == 300           # LMeDS's fixed count
    assert R.update_num_iters(0.99, 0.9, 7, 1000) == 1000           # capped by maxIters
    assert R.update_num_iters(0.99, 0.5, 7, 200) == 200


def test_solve_cubic_known_roots():
    n, r = R.solve_cubic([1.0, -6.0, 11.0, -6.0])                   # (x-1)(x-2)(x-3)
    assert n == 3 and sorted(round(v, 12) for v in r) == [1.0, 2.0, 3.0]
    n, r = R.solve_cubic([1.0, 0.0, 0.0, -8.0])                     # x^3 = 8
    assert n == 1 and abs(r[0] - 2.0) < 1e-12
    n, r = R.solve_cubic([0.0, 1.0, -3.0, 2.0])                     # quadratic (x-1)(x-2)
    assert n == 2 and sorted(r[:2]) == [1.0, 2.0]
    assert R.solve_cubic([0.0, 0.0, 0.0, 0.0])[0] == -1


# ---- two-view known answers -------------------------------------------------------------------------
def test_seven_exact_correspondences_give_the_true_F():
    for seed in range(5):
        p1, p2, _, (Rm, t) = R.two_view(7, seed=seed)
        Ft = R.true_F(Rm, t)
        Ft = (Ft / Ft[2, 2]).ravel()
        cands = R.run7point(p1, p2)
        assert 1 <= len(cands) <= 3
        err = min(np.abs(np.array(F) - Ft).max() / np.abs(Ft).max() for F in cands)
        assert err < 1e-3, (seed, err)
        st, T = R.find(p1, p2, 1.0)
        assert T["path"] == "kernel" and st.tolist() == [1] * 7


@pytest.mark.parametrize("outliers", [0.1, 0.3, 0.5])
def test_planted_outliers_are_rejected(outliers):
    for seed in range(3):
        p1, p2, truth, _ = R.two_view(150, outliers, 0.0, seed=seed)
        st, T = R.find(p1, p2, 1.0)
        assert T["path"] == "ransac"
        assert st.astype(bool).tolist() == truth.tolist(), seed      # exact geometry: inliers all kept, outliers all gone
        p1, p2, truth, _ = R.two_view(150, outliers, 0.3, seed=seed)
        st, _ = R.find(p1, p2, 1.0)
        assert not st[~truth].any(), seed                              # 15..60 px jumps never pass a 1 px threshold
        # a 7-point model without refit keeps most, not all, of the inliers under 0.3 px noise
        assert st[truth].mean() >= 0.8, (seed, st[truth].mean())


@pytest.mark.parametrize("n", list(range(8, 16)))
def test_path_choice(n):
    p1, p2, _, _ = R.two_view(n, seed=n)
    st, T = R.find(p1, p2, 1.0)
    if n < 15:
        assert T["path"] == "lmeds" and T["niters0"] == 300 and T["iters"] == 300
    else:
        assert T["path"] == "ransac" and T["niters0"] == 1000
    assert T["best_iter"] >= 0 and st.sum() >= 7


def test_zero_motion_keeps_every_point():
    for n in (10, 150):
        p1, _, _, _ = R.two_view(n, seed=3)
        st, T = R.find(p1, p1.copy(), 1.0)
        assert st.all(), (n, T["path"])


def test_all_collinear_exhausts_get_subset():
    for n in (12, 40):
        k = np.arange(n)
        p1 = np.c_[50 + 8 * k, 100 + 2 * k].astype(np.float32)          # exactly on one line
        p2 = (p1 + np.float32(3)).astype(np.float32)
        st, T = R.find(p1, p2, 1.0)
        assert T["n_subsets"] == 0 and T["best_iter"] == -1 and not st.any()
        # the switch: without checkSubset the same stream yields subsets (whose 7x9 system is rank deficient)
        st0, T0 = R.find(p1, p2, 1.0, check=0)
        assert T0["n_subsets"] > 0


def test_threshold_is_rounded_to_float_once():
    p1, p2, _, _ = R.two_view(40, 0.2, 0.5, seed=11)
    st, T = R.find(p1, p2, 1.0)
    e = R.errors(T["F_best"], p1, p2)
    assert (st == (e <= np.float32(1.0))).all()
    assert T["n_inliers"] == int(st.sum())


def test_lmeds_sigma_floor():
    assert R.lmeds_sigma(10, 0.0) == 0.001
    assert math.isclose(R.lmeds_sigma(12, 1.0), 2.5 * 1.4826 * 2.0)


def test_lmeds_medians_below_fourteen_points_are_rounding_noise():
    """n <= 13: n/2 < 7, so every candidate's median is one of the 7 errors it fits exactly"""
    for n in (8, 11, 13):
        p1, p2, _, _ = R.two_view(n, 0.0, 0.0, seed=40 + n)
        _, T = R.find(p1, p2, 1.0)
        assert T["path"] == "lmeds" and T["best_median"] < 1e-20, (n, T["best_median"])
    p1, p2, _, _ = R.two_view(14, 0.3, 0.3, seed=54)
    _, T = R.find(p1, p2, 1.0)
    assert T["best_median"] > 1e-12                                   # n = 14: the 8th smallest error, a real residual
    sc = np.array([[5, 0, 0], [7, 9, 0]])
    assert R.lmeds_rounding_decided("lmeds", 8, (1, 1), (0, 0), sc, np.array([[5, 0, 0], [7, 8, 0]]))
    assert not R.lmeds_rounding_decided("lmeds", 8, (1, 1), (0, 0), sc, sc)
    assert not R.lmeds_rounding_decided("lmeds", 14, (1, 1), (0, 0), sc, np.array([[5, 0, 0], [7, 8, 0]]))
    assert not R.lmeds_rounding_decided("ransac", 8, (1, 1), (0, 0), sc, np.array([[5, 0, 0], [7, 8, 0]]))


# ---- the host half of csrc/lvi_ransac.hpp under the host sanitizers ---------------------------------------------
DRIVER = r"""
// stand-alone driver of the 7-point sample stream of lvi_fmat_find (csrc/lvi_ransac.hpp, no HIP)
//   driver FILE n lmeds|ransac max_iters confidence check      FILE: n x (x1 y1 x2 y2) float
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "lvi_ransac.hpp"
using namespace lvi_ransac;

int main(int argc, char** argv)
{
    if (argc < 7) return 1;
    const int n = std::atoi(argv[2]), max_iters = std::atoi(argv[4]), check = std::atoi(argv[6]);
    const bool ransac = !std::strcmp(argv[3], "ransac");
    const double confidence = std::atof(argv[5]);
    std::vector<float> xy(4 * (size_t)n);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(xy.data(), 4, xy.size(), f) != xy.size()) return 2;
    std::fclose(f);
    // as lvi_fmat_find calls it, into the room a handle of max_iters has and no more
    std::vector<int32_t> sub(7 * (size_t)max_iters), again(sub.size());
    int niters0 = 0;
    const int nsub = fm_sample_stream(xy.data(), n, ransac, max_iters, confidence, check, sub.data(), &niters0);
    // the same stream once more through a predicate that counts the subsets getSubset drew
    long attempts = 0;
    const int nsub2 = sample_stream<7>(n, niters0, ransac ? FM_RANSAC_MAX_ATTEMPTS : FM_LMEDS_MAX_ATTEMPTS,
                                       [&](const int32_t* idx) { attempts++; return fm_check_subset(xy.data(), idx, check); }, again.data());
    if (nsub2 != nsub || std::memcmp(sub.data(), again.data(), sizeof(int32_t) * 7 * (size_t)nsub)) return 3;
    std::printf("niters0 %d\nattempts %ld\n", niters0, attempts);
    for (int h = 0; h < nsub; h++) {
        std::printf("sub");
        for (int k = 0; k < 7; k++) std::printf(" %d", sub[7 * h + k]);
        std::printf("\n");
    }
    const int gs[5] = {0, 1, n / 2, n - 1, n};
    for (int g : gs) std::printf("log %d %a\n", g, update_log<7>(n, g));
    return 0;
}
"""


def _collinear40():
    k = np.arange(40)
    p1 = np.c_[50 + 8 * k, 100 + 2 * k].astype(np.float32)               # test_collinear_set_gives_no_model_and_the_switch's points
    return p1, p1 + np.float32(3)


def _stream_cases():
    tv = lambda n, **kw: R.two_view(n, 0.3, 0.3, seed=n, **kw)[:2]
    return [("lmeds8", tv(8), 1000, 1), ("lmeds14", tv(14), 1000, 1), ("ransac15", tv(15), 1000, 1), ("ransac150", tv(150), 1000, 1),
            ("duplicates150", tv(150, kind="duplicates"), 1000, 1), ("collinear40", _collinear40(), 1000, 1), ("collinear40_unchecked", _collinear40(), 1000, 0),
            ("lmeds8_max1", tv(8), 1, 1), ("lmeds8_max2", tv(8), 2, 1), ("ransac2500", tv(2500), 1000, 1)]


@pytest.fixture(scope="module")
def stream_drivers(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("fmat_stream")
    (d / "driver.cpp").write_text(DRIVER)
    out = {}
    for which, flags in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        out[which] = str(d / which)
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", *flags, "-I" + os.path.join(pkg.PKG_DIR, "csrc"), "-o", out[which],
                            str(d / "driver.cpp")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return out


@pytest.fixture(scope="module")
def stream_wants():
    """fmat_ref.sample_stream per case, computed once for both builds -> (subsets, niters0, attempts)"""
    out = {}
    for name, (p1, p2), max_iters, check in _stream_cases():
        attempts = [0]
        subs, niters0 = R.sample_stream(p1, p2, len(p1), R.choose_path(len(p1)), max_iters, 0.99, check, attempts)
        out[name] = (subs, niters0, attempts[0])
    return out


@pytest.mark.parametrize("which", ["plain", "san"])
def test_seven_point_stream_equals_the_restatement(stream_drivers, stream_wants, tmp_path, which):
    """csrc/lvi_ransac.hpp as lvi_fmat_find calls it, run as a child process: the subsets, the count asked for and the
    number of subsets getSubset drew are fmat_ref.sample_stream's, integer for integer; update_log<7> gives
    fmat_ref.update_num_iters"""
    seen = {}
    for name, (p1, p2), max_iters, check in _stream_cases():
        n = len(p1)
        path = R.choose_path(n)
        (tmp_path / "xy.bin").write_bytes(np.c_[p1, p2].astype(np.float32).tobytes())
        r = subprocess.run([stream_drivers[which], str(tmp_path / "xy.bin"), str(n), path, str(max_iters), "0.99", str(check)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stdout[-300:] + r.stderr)
        lines = [l.split() for l in r.stdout.split("\n") if l]
        subs = [list(map(int, l[1:])) for l in lines if l[0] == "sub"]
        niters0 = [int(l[1]) for l in lines if l[0] == "niters0"]
        attempts = [int(l[1]) for l in lines if l[0] == "attempts"]
        logs = {int(l[1]): float.fromhex(l[2]) for l in lines if l[0] == "log"}
        want_subs, want_niters0, want_attempts = stream_wants[name]
        assert subs == want_subs and niters0 == [want_niters0] and attempts == [want_attempts], name
        seen[name] = (len(subs), niters0[0], attempts[0])
        assert sorted(logs) == sorted({0, 1, n // 2, n - 1, n}) and logs[n] == float("inf")   # ep = 0: denom < DBL_MIN
        assert R.update_num_iters(0.99, 0.0, 7, 1000) == 0
        num = np.log(max(1.0 - 0.99, R.DBL_MIN))
        for g in (0, 1, n // 2, n - 1):
            # recomputed from the table as the device walk does
            got = 1000 if logs[g] >= 0 or -num >= 1000 * -logs[g] else int(round(num / logs[g]))
            assert got == R.update_num_iters(0.99, (n - g) / n, 7, 1000), (name, g)
    # what each case is there for
    assert seen["lmeds8"][:2] == seen["lmeds14"][:2] == (300, 300)                       # update_num_iters(0.99, 0.45, 7, I), floor 3
    assert seen["ransac15"][:2] == seen["ransac150"][:2] == seen["ransac2500"][:2] == (1000, 1000)
    assert seen["duplicates150"][0] == 1000 and seen["duplicates150"][2] > 1000         # checkSubset rejected subsets inside the stream
    assert seen["collinear40"] == (0, 1000, R.RANSAC_MAX_ATTEMPTS)                      # no subset, and only after every attempt
    assert seen["collinear40_unchecked"] == (1000, 1000, 1000)
    assert seen["lmeds8_max1"][:2] == (1, 1) and seen["lmeds8_max2"][:2] == (2, 2)       # min(niters0, I) under LMeDS's floor of 3
