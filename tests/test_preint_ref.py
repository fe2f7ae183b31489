"""CPU tier of the IMU preintegration (include/lvi_preint.h): the ABI checks, tests/preint_ref.py in float64
against itself in mpmath and against the independent numpy statement tests/win_ref.py::preintegrate,
csrc/lvi_preint_math.hpp compiled alone (plain and as a stand-alone program under the host sanitizers) bit for bit against
the float64 reference, and the invariants of the reference's operations on random sequences."""
import copy
import ctypes
import importlib
import os
import re
import subprocess

import mpmath
import numpy as np
import pytest

import preint_ref as R
import win_ref as W
import win_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("sum_dt", "delta_p", "delta_q", "delta_v", "linearized_ba", "linearized_bg", "jacobian", "covariance")

# The bar of the float64 reference against mpmath, per field, as a fraction of the field's largest magnitude: four times the
# largest error of the parent's win_ref.preintegrate against the same mpmath values on the same sequences (`_cases`).  Both
# are rounding-level; they differ in summation order and in skipping structural zeros, which is what the factor covers.
# Measured, win_ref.preintegrate / preint_ref: sum_dt 4.51e-16 / 4.51e-16, delta_p 3.03e-16 / 3.84e-16, delta_q
# 1.38e-16 / 1.89e-16, delta_v 4.65e-16 / 2.66e-16, linearized_ba and _bg 0 / 0, jacobian 3.75e-16 / 3.75e-16, covariance
# 1.32e-15 / 1.32e-15.
WIN_REF_ERROR = dict(sum_dt=4.510e-16, delta_p=3.032e-16, delta_q=1.377e-16, delta_v=4.654e-16, linearized_ba=0.0, linearized_bg=0.0, jacobian=3.750e-16,
                     covariance=1.323e-15)
BAR = {k: 4.0 * v for k, v in WIN_REF_ERROR.items()}


def _header():
    return open(os.path.join(ROOT, "include", "lvi_preint.h")).read()


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(lvi_preint_[a-z0-9_]+)\s*\(", txt)))


# ---- ABI -------------------------------------------------------------------------------------------
def test_header_and_preint_binding_agree(pkg):
    P = pkg.preint
    assert _declared() == sorted(P.PREINT_SIGNATURES.keys())
    assert len(_declared()) == 15
    for other in (pkg._abi.SIGNATURES, pkg.marg.MARG_SIGNATURES, pkg.win.WIN_SIGNATURES, pkg.fman.FMAN_SIGNATURES):
        assert not set(_declared()) & set(other)
    txt = _header()
    for name, val in (("ABI_VERSION", 1), ("SLOTS", P.SLOTS), ("MAX_SAMPLES", P.MAX_SAMPLES), ("CHUNK", P.CHUNK)):
        assert int(re.search(r"#define LVI_PREINT_%s\s+(\d+)" % name, txt).group(1)) == val, name
    assert (P.SLOTS, P.MAX_SAMPLES, P.CHUNK, P.WINDOW) == (11, 8192, R.CHUNK, R.WINDOW) and (R.SLOTS, R.MAX_SAMPLES) == (P.SLOTS, P.MAX_SAMPLES)
    # every entry point cites the lines it restates
    assert all(s in txt for s in ("estimator.cpp:82-116", "integration_base.h:9-158", ":215-269", ":988-1016", ":1043-1068", ":38-52", ":84-89", ":91-94",
                                  ":95-113", ":740", "imu_factor.h:18-178", ":21-27"))
    # the record type is the window solve's, included and not copied
    assert '#include "lvi_win.h"' in txt and "lvi_preint_imu" not in txt and "typedef struct lvi_win_imu" not in txt
    assert P.ImuWindow.imu_dtype is pkg.win.IMU_DTYPE and pkg.win.IMU_DTYPE.itemsize == ctypes.sizeof(pkg.win.WinImu) == 3752
    for other in ("lvi_hotpath.h", "lvi_marg.h", "lvi_win.h", "lvi_fman.h"):
        assert "lvi_preint" not in open(os.path.join(ROOT, "include", other)).read(), other
    # the host header stays out of the oracle-linked mirror
    host = os.path.join(pkg.PKG_DIR, "host")
    for f in ("lvi_host.hpp", "lvi_seq_capi.cpp"):
        assert "lvi_preint" not in open(os.path.join(host, f)).read(), f
    assert not any(f.startswith("lvi_preint") and f.endswith(".cpp") for f in os.listdir(host))
    assert "preint" not in pkg.host_api.COMPONENTS


def test_record_layouts(pkg):
    P = pkg.preint
    txt = _header()
    for cname, cls, size in (("lvi_preint_caps", P.PreintCaps, 8), ("lvi_preint_params", P.PreintParams, 56), ("lvi_preint_nav", P.PreintNav, 168)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in re.findall(r"\b(?:int32_t|double)\s+([^;]+);", body) for n in re.findall(r"([A-Za-z_][A-Za-z_0-9]*)(?:\[\d+\])?\s*(?:,|$)", decl)]
        assert names == [f[0] for f in cls._fields_], cname
        assert ctypes.sizeof(cls) == size, cname
    assert [(f[0], getattr(P.PreintNav, f[0]).offset) for f in P.PreintNav._fields_] == [("P", 0), ("R", 24), ("V", 96), ("Ba", 120), ("Bg", 144)]
    assert P.PreintParams.G.offset == 32


def test_hip_library_exports_the_preint_abi_and_the_oracle_does_not(pkg, oracle):
    dll = ctypes.CDLL(pkg.HIP_LIB_PATH)
    for name in _declared():
        assert hasattr(dll, name), f"{name} missing from liblvi_hip.so"
    lib = pkg.preint.bind(pkg.load_hip())
    assert lib.dll.lvi_preint_abi_version() == 1 and lib.dll.lvi_win_abi_version() == 1 and lib.dll.lvi_abi_version() == 6
    p = pkg.preint.PreintParams()
    lib.dll.lvi_preint_params_default(ctypes.byref(p))
    assert (p.acc_n, p.gyr_n, p.acc_w, p.gyr_w, tuple(p.G)) == tuple(R.PARAMS[k] for k in ("acc_n", "gyr_n", "acc_w", "gyr_w", "G")) == \
        (0.08, 0.004, 4e-5, 2e-6, (0.0, 0.0, 9.8))
    w = pkg.win.WinParams()
    pkg.win.bind(lib).dll.lvi_win_params_default(ctypes.byref(w))
    assert tuple(w.G) == tuple(p.G)
    syms = subprocess.run(["nm", "-D", "--defined-only", oracle.path], capture_output=True, text=True).stdout
    assert "lvi_abi_version" in syms and "lvi_preint_" not in syms
    syms = subprocess.run(["nm", "-D", "--defined-only", pkg.host_api.HOST_HIP_LIB], capture_output=True, text=True).stdout
    assert "lvh_" in syms and "preint" not in syms
    b = importlib.import_module(pkg.__name__ + ".build")
    assert "lvi_preint.hip" in b.SOURCES and os.path.join(ROOT, "include", "lvi_preint.h") in b.hip_dependencies()


def test_imu_window_fails_loudly_without_gpu(pkg):
    """no CPU fallback: without a device the handle is refused; arguments are refused before the device is looked for"""
    import torch
    lib = pkg.load_hip()
    for bad in (0, pkg.preint.MAX_SAMPLES + 1):
        with pytest.raises(pkg.LviError) as e:
            pkg.ImuWindow(lib, max_samples=bad)
        assert e.value.code == pkg._abi.LVI_ERR_INVALID_ARG
    if not torch.cuda.is_available():
        with pytest.raises(pkg.LviError) as e:
            pkg.ImuWindow(lib, max_samples=64)
        assert e.value.code == pkg._abi.LVI_ERR_NO_DEVICE


# ---- the reference in float64 against mpmath and against win_ref.preintegrate ---------------------------------------
def _cases():
    """(name, dt, acc, gyr, ba, bg): 1, 2, 6 and 40 steps (the first sample initialises acc_0 and gyr_0); dt constant, varying,
    and varying with one dt == 0 step; zero and non-zero biases"""
    out = []
    for steps in (1, 2, 6, 40):
        for ki, kind in enumerate(("const", "vary", "zero")):
            for bias in (0, 1):
                seed = 100 * steps + 10 * ki + bias
                dt, acc, gyr = R.samples(seed, steps + 1, vary=kind != "const", zero_dt_at=min(steps, 3) if kind == "zero" else None)
                rs = np.random.RandomState(seed + 7)
                ba, bg = (rs.normal(0, 0.02, 3), rs.normal(0, 0.002, 3)) if bias else (np.zeros(3), np.zeros(3))
                out.append((f"{steps}-{kind}-{bias}", dt, acc, gyr, ba, bg))
    return out


def _scaled_error(f64, mp):
    m = np.asarray(mp, dtype=object).reshape(-1)
    scale = max(abs(float(v)) for v in m) or 1.0
    return max(abs(float(mpmath.mpf(float(a)) - b)) for a, b in zip(np.asarray(f64, np.float64).reshape(-1), m)) / scale


def test_float64_reference_against_mpmath():
    worst_new, worst_old = {k: 0.0 for k in FIELDS}, {k: 0.0 for k in FIELDS}
    for name, dt, acc, gyr, ba, bg in _cases():
        mp = R.exact_record(R.preintegrate(dt, acc, gyr, ba, bg, R.MP))
        new = R.to_record(R.preintegrate(dt, acc, gyr, ba, bg, R.F64))
        old = W.preintegrate(list(dt), list(acc), list(gyr), ba, bg)
        for k in FIELDS:
            worst_new[k] = max(worst_new[k], _scaled_error(new[k], mp[k]))
            worst_old[k] = max(worst_old[k], _scaled_error(old[k], mp[k]))
    for k in FIELDS:
        print(f"[preint ref] {k}: win_ref.preintegrate {worst_old[k]:.3e}, preint_ref {worst_new[k]:.3e}, bar {BAR[k]:.3e}")
    for k in FIELDS:
        assert worst_new[k] <= BAR[k], k
        assert abs(worst_old[k] - WIN_REF_ERROR[k]) <= 1e-3 * WIN_REF_ERROR[k], k      # the column the bar is built from still stands
    assert any("zero" in c[0] and 0.0 in c[1][1:] for c in _cases())           # a dt == 0 step is among them


@pytest.mark.parametrize("seed", [1, 6, 31])
def test_float64_reference_against_win_ref_preintegrate(seed):
    """two independent statements of the same formulas on the samples win_scenes.make_scene draws: their distance to the same
    bar, scaled by the field's largest magnitude"""
    ba, bg, intervals = R.scene_intervals(seed, 4)
    sc = S.make_scene(seed, 4, [4] * 3)
    recs = [op[1] for op in sc["ops"] if op[0] == "imu"]
    assert len(recs) == len(intervals) == 3
    worst = {k: 0.0 for k in FIELDS}
    for (dts, accs, gyrs, p), rec in zip(intervals, recs):
        assert all(np.array_equal(np.asarray(p[k]), np.asarray(rec[k])) for k in FIELDS)      # the samples are make_scene's
        new = R.to_record(R.preintegrate(dts, accs, gyrs, ba, bg))
        mp = R.exact_record(R.preintegrate(dts, accs, gyrs, ba, bg, R.MP))
        for k in FIELDS:
            scale = float(np.abs(np.asarray(p[k])).max()) or 1.0
            worst[k] = max(worst[k], float(np.abs(np.asarray(new[k]) - np.asarray(p[k])).max()) / scale)
            assert _scaled_error(new[k], mp[k]) <= BAR[k], k
    print(f"[preint ref] seed {seed}: preint_ref against win_ref.preintegrate {({k: f'{v:.2e}' for k, v in worst.items()})}")
    for k in FIELDS:
        assert worst[k] <= BAR[k], k


# ---- csrc/lvi_preint_math.hpp alone, plain and under the host sanitizers -----------------------------------------
DRIVER = r"""
// stand-alone driver of csrc/lvi_preint_math.hpp: the chain as the kernel runs it, on the host
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lvi_preint_math.hpp"
using namespace lvi_preint_math;
int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    double head[41];     // n, ba, bg, acc_0, gyr_0, acc_n, gyr_n, acc_w, gyr_w, G, nav (21)
    while (fread(head, sizeof(double), 41, f) == 41) {
        const int n = (int)head[0];
        if (n < 0 || n > 100000) return 4;
        std::vector<double> smp((size_t)n * 7), dt((size_t)n), acc((size_t)n * 3), gyr((size_t)n * 3);
        if (fread(smp.data(), sizeof(double), smp.size(), f) != smp.size()) return 5;
        for (int k = 0; k < n; k++) {
            dt[k] = smp[7 * k];
            for (int a = 0; a < 3; a++) { acc[3 * k + a] = smp[7 * k + 1 + a]; gyr[3 * k + a] = smp[7 * k + 4 + a]; }
        }
        State s;
        state_reset(s, head + 7, head + 10, head + 1, head + 4);
        std::vector<double> J(225), C(225), work(WORK_DOUBLES);
        matrices_reset(J.data(), C.data());
        double q[NV];
        noise_diag(head[13], head[14], head[15], head[16], q);
        Nav nav;
        for (int k = 0; k < 21; k++) (&nav.P[0])[k] = head[20 + k];
        double e_acc[3] = {head[7], head[8], head[9]}, e_gyr[3] = {head[10], head[11], head[12]};
        for (int k = 0; k < n; k++) {
            nav_step(nav, e_acc, e_gyr, dt[k], &acc[3 * k], &gyr[3 * k], head + 17);
            for (int a = 0; a < 3; a++) { e_acc[a] = acc[3 * k + a]; e_gyr[a] = gyr[3 * k + a]; }
        }
        // half of the samples through integrate(), the rest one call each: the same chain
        const int h = n / 2;
        integrate(s, J.data(), C.data(), q, h, dt.data(), acc.data(), gyr.data(), work.data());
        for (int k = h; k < n; k++) integrate(s, J.data(), C.data(), q, 1, &dt[k], &acc[3 * k], &gyr[3 * k], work.data());
        printf("%a", s.sum_dt);
        for (int k = 0; k < 3; k++) printf(" %a", s.delta_p[k]);
        for (int k = 0; k < 4; k++) printf(" %a", s.delta_q[k]);
        for (int k = 0; k < 3; k++) printf(" %a", s.delta_v[k]);
        for (int k = 0; k < 3; k++) printf(" %a", s.linearized_ba[k]);
        for (int k = 0; k < 3; k++) printf(" %a", s.linearized_bg[k]);
        for (int k = 0; k < 225; k++) printf(" %a", J[k]);
        for (int k = 0; k < 225; k++) printf(" %a", C[k]);
        for (int k = 0; k < 21; k++) printf(" %a", (&nav.P[0])[k]);
        printf("\n");
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
    d = tmp_path_factory.mktemp("preint_header")
    return {"plain": _build_driver(pkg, d / "plain", []),
            "san": _build_driver(pkg, d / "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])}


NAV0 = dict(P=[0.3, -0.1, 0.2], R=W.M.rot(np.array([0.1, -0.05, 0.02, 0.99])).ravel(), V=[1.5, 0.2, -0.1], Ba=[0.01, -0.02, 0.015], Bg=[0.001, 0.002, -0.0015])


@pytest.fixture(scope="module")
def header_reference():
    """the float64 reference of every case, computed once: (blob, [(record, nav)])"""
    blob, want = b"", []
    for name, dt, acc, gyr, ba, bg in _cases():
        est = R.Estimator()
        est.set_nav(NAV0["P"], NAV0["R"], NAV0["V"], ba, bg)
        est.push(0, dt[:1], acc[:1], gyr[:1])              # the first sample: acc_0, gyr_0
        est.push(1, dt[1:], acc[1:], gyr[1:])
        nav = est.nav_f64()
        want.append((est.record(1), np.r_[nav["P"], nav["R"].ravel(), nav["V"], nav["Ba"], nav["Bg"]]))
        n = len(dt) - 1
        head = np.r_[float(n), ba, bg, acc[0], gyr[0], [R.PARAMS[k] for k in ("acc_n", "gyr_n", "acc_w", "gyr_w")], R.PARAMS["G"], NAV0["P"], NAV0["R"],
                     NAV0["V"], ba, bg]
        blob += head.astype(np.float64).tobytes() + np.c_[dt[1:], acc[1:], gyr[1:]].astype(np.float64).tobytes()
    return blob, want


@pytest.mark.parametrize("which", ["plain", "san"])
def test_math_header_equals_the_float64_reference_bit_for_bit(drivers, header_reference, tmp_path, which):
    """only IEEE + - * / sqrt in a stated order with contraction off: no tolerance; the sanitizer build must exit clean"""
    blob, want = header_reference
    (tmp_path / "s.bin").write_bytes(blob)
    out = subprocess.run([drivers[which], str(tmp_path / "s.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l.split() for l in out.stdout.split("\n") if l]
    assert len(lines) == len(want) == 24
    for (name, *_), line, (rec, nav) in zip(_cases(), lines, want):
        v = np.array([float.fromhex(t) for t in line])
        assert len(v) == 1 + 3 + 4 + 3 + 3 + 3 + 225 + 225 + 21
        got = dict(sum_dt=v[0], delta_p=v[1:4], delta_q=v[4:8], delta_v=v[8:11], linearized_ba=v[11:14], linearized_bg=v[14:17], jacobian=v[17:242].reshape(15, 15),
                   covariance=v[242:467].reshape(15, 15))
        assert R.same_record(got, rec) is None, (which, name, R.same_record(got, rec))
        assert np.array_equal(v[467:], nav), (which, name, "nav")
    print(f"[preint header] {which}: {len(want)} sequences, every field of the record and the navigation state equal the float64 reference bit for bit")


# ---- the host model's invariants on random operation sequences -----------------------------------------------------
def _concat(a, b):
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_operation_sequences_keep_the_invariants(seed):
    rs = np.random.RandomState(seed)
    cap = 40
    est, frame_count, seen = R.Estimator(max_samples=cap), 0, set()
    ops = ["old", "new", "repropagate", "new", "new", "old", "repropagate", "new", "clear"]
    for image in range(32):
        n = int(rs.randint(1, 9))
        dt, acc, gyr = R.samples(1000 * seed + image, n, vary=True)
        # chunked pushes equal one push
        twin = copy.deepcopy(est)
        cut = int(rs.randint(0, n + 1))
        try:
            est.push(frame_count, dt, acc, gyr)
        except R.CapacityError:
            seen.add("capacity")
            est.slide_old()
            continue
        twin.push(frame_count, dt[:cut], acc[:cut], gyr[:cut])
        twin.push(frame_count, dt[cut:], acc[cut:], gyr[cut:])
        assert R.same_record(est.record(frame_count), twin.record(frame_count)) is None
        assert all(np.array_equal(est.nav_f64()[k], twin.nav_f64()[k]) for k in ("P", "R", "V"))
        if frame_count == 0:
            assert est.slots[0]["samples"] == [] and est.record(0)["sum_dt"] == 0.0
        if frame_count < R.WINDOW:
            frame_count += 1
            continue
        # repropagate with a slot's own biases reproduces its record bit for bit
        before = [est.record(i) for i in range(R.SLOTS)]
        Bas, Bgs = np.array([r["linearized_ba"] for r in before]), np.array([r["linearized_bg"] for r in before])
        est.repropagate(Bas, Bgs)
        assert all(R.same_record(est.record(i), before[i]) is None for i in range(R.SLOTS))
        what = ops.pop(0) if ops else "old"
        if what == "old":
            old = [est.record(i) for i in range(R.SLOTS)]
            est.slide_old()
            assert all(R.same_record(est.record(i), old[i + 1]) is None for i in range(R.WINDOW))
            assert est.record(R.WINDOW)["sum_dt"] == 0.0 and est.slots[R.WINDOW]["samples"] == []
            seen.add("old")
        elif what == "new":
            s9, s10 = est.samples(9), est.samples(10)
            try:
                est.slide_new()
            except R.CapacityError:
                seen.add("capacity")
                est.slide_old()
                continue
            got = est.samples(9)
            assert all(np.array_equal(a, b) for a, b in zip(got, _concat(s9, s10)))        # its old ones followed by slot 10's
            assert est.slots[10]["samples"] == []
            seen.add("new")
        elif what == "repropagate":
            slots = sorted(set(rs.randint(0, R.SLOTS, 3).tolist()))
            B1, B2 = Bas + rs.normal(0, 1e-3, Bas.shape), Bgs + rs.normal(0, 1e-4, Bgs.shape)
            est.repropagate(B1, B2, slots)
            for i in range(R.SLOTS):
                if i in slots:
                    assert np.array_equal(est.record(i)["linearized_ba"], B1[i]) and est.record(i)["sum_dt"] == before[i]["sum_dt"]
                else:
                    assert R.same_record(est.record(i), before[i]) is None
            seen.add("repropagate")
        else:
            est.clear()
            assert all(s is None for s in est.slots) and not est.first_imu
            frame_count = 0
            seen.add("clear")
    assert {"old", "new", "repropagate", "clear"} <= seen and not ops, (seen, ops)
