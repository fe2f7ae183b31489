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
