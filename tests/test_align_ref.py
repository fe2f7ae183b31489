"""CPU tier of the visual-inertial alignment (include/lvi_align.h): the ABI checks, tests/align_ref.py against
itself (band = dense), against numpy.linalg.solve and against mpmath, csrc/lvi_align_math.hpp compiled alone into a
stand-alone program (plain and under the host sanitizers) bit for bit against the float64 reference, the recovery of the
truth on analytic preintegrations, the branches, and the tail of visualInitialAlign."""
import ctypes
import importlib
import os
import re
import subprocess

import mpmath
import numpy as np
import pytest

import align_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDED = [(seed, F) for F in (4, 5, 11) for seed in (1, 2, 3)] + [(4, 30)]      # (seed, frames) of the seeded scenes
U = 2.22e-16


def _header():
    return open(os.path.join(ROOT, "include", "lvi_align.h")).read()


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(lvi_align_[a-z0-9_]+)\s*\(", txt)))


# ---- ABI -------------------------------------------------------------------------------------------
def test_header_and_align_binding_agree(pkg):
    P = pkg.align
    assert _declared() == sorted(P.ALIGN_SIGNATURES.keys()) and len(_declared()) == 16
    for other in (pkg._abi.SIGNATURES, pkg.marg.MARG_SIGNATURES, pkg.win.WIN_SIGNATURES, pkg.fman.FMAN_SIGNATURES, pkg.preint.PREINT_SIGNATURES,
                  pkg.relpose.RELPOSE_SIGNATURES):
        assert not set(_declared()) & set(other)
    txt = _header()
    for name, val in (("ABI_VERSION", 1), ("MAX_FRAMES", P.MAX_FRAMES), ("SYSTEMS", P.SYSTEMS), ("OK", P.OK), ("GRAVITY_NORM", P.GRAVITY_NORM),
                      ("NEGATIVE_SCALE", P.NEGATIVE_SCALE), ("NEGATIVE_SCALE_REFINED", P.NEGATIVE_SCALE_REFINED), ("SINGULAR", P.SINGULAR), ("TOO_FEW", P.TOO_FEW),
                      ("APPLY_OPPOSITE", P.APPLY_OPPOSITE)):
        assert int(re.search(r"#define LVI_ALIGN_%s\s+(\d+)" % name, txt).group(1)) == val, name
    assert (P.OK, P.GRAVITY_NORM, P.NEGATIVE_SCALE, P.NEGATIVE_SCALE_REFINED, P.SINGULAR, P.TOO_FEW) == \
        (R.OK, R.GRAVITY_NORM, R.NEGATIVE_SCALE, R.NEGATIVE_SCALE_REFINED, R.SINGULAR, R.TOO_FEW)
    assert all(s in txt for s in ("estimator.cpp:99", ":132-135", ":1019-1033", ":273-300", "initial_aligment.cpp:3-209", ":450-486", ":48-50", ":339-410", ":434"))
    assert "IS NOT COMPUTED" in txt and '#include "lvi_preint.h"' in txt
    for other in ("lvi_hotpath.h", "lvi_marg.h", "lvi_win.h", "lvi_fman.h", "lvi_preint.h", "lvi_relpose.h"):
        assert "lvi_align" not in open(os.path.join(ROOT, "include", other)).read(), other
    host = os.path.join(pkg.PKG_DIR, "host")
    for f in ("lvi_host.hpp", "lvi_seq_capi.cpp"):
        assert "lvi_align" not in open(os.path.join(host, f)).read(), f
    assert "align" not in pkg.host_api.COMPONENTS and pkg.ImuAligner is P.ImuAligner


def test_record_layouts(pkg):
    P = pkg.align
    txt = _header()
    for cname, cls, size in (("lvi_align_caps", P.AlignCaps, 8), ("lvi_align_params", P.AlignParams, 80), ("lvi_align_info", P.AlignInfo, 144),
                             ("lvi_align_frame", P.AlignFrame, 2104)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in re.findall(r"\b(?:int32_t|double)\s+([^;]+);", body) for n in re.findall(r"([A-Za-z_][A-Za-z_0-9]*)(?:\[\d+\])?\s*(?:,|$)", decl)]
        assert names == [f[0] for f in cls._fields_], cname
        assert ctypes.sizeof(cls) == size, cname


def test_hip_library_exports_the_align_abi_and_the_oracle_does_not(pkg, oracle):
    dll = ctypes.CDLL(pkg.HIP_LIB_PATH)
    for name in _declared():
        assert hasattr(dll, name), f"{name} missing from liblvi_hip.so"
    lib = pkg.align.bind(pkg.load_hip())
    assert lib.dll.lvi_align_abi_version() == 1 and lib.dll.lvi_abi_version() == 6
    p = pkg.align.AlignParams()
    lib.dll.lvi_align_params_default(ctypes.byref(p))
    assert (p.acc_n, p.gyr_n, p.acc_w, p.gyr_w, tuple(p.G), tuple(p.TIC)) == tuple(R.PARAMS[k] for k in ("acc_n", "gyr_n", "acc_w", "gyr_w", "G", "TIC"))
    syms = subprocess.run(["nm", "-D", "--defined-only", oracle.path], capture_output=True, text=True).stdout
    assert "lvi_abi_version" in syms and "lvi_align_" not in syms
    b = importlib.import_module(pkg.__name__ + ".build")
    assert "lvi_align.hip" in b.SOURCES and os.path.join(ROOT, "include", "lvi_align.h") in b.hip_dependencies()


def test_imu_aligner_fails_loudly_without_gpu(pkg):
    import torch
    lib = pkg.load_hip()
    for kw in (dict(max_frames=1), dict(max_frames=pkg.align.MAX_FRAMES + 1), dict(max_samples=0)):
        with pytest.raises(pkg.LviError) as e:
            pkg.ImuAligner(lib, **kw)
        assert e.value.code == pkg._abi.LVI_ERR_INVALID_ARG
    if not torch.cuda.is_available():
        with pytest.raises(pkg.LviError) as e:
            pkg.ImuAligner(lib, max_frames=8, max_samples=16)
        assert e.value.code == pkg._abi.LVI_ERR_NO_DEVICE


def test_apply_on_the_host_needs_no_device(pkg):
    """lvi_align_apply is a host function of the library: it runs on a machine without a GPU"""
    lib = pkg.align.bind(pkg.load_hip())
    case = _apply_case(7, False)
    got = _apply_lib(pkg, lib, case)
    _check_apply(case, got, "library")


# ---- scenes, computed once -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solved():
    """every seeded scene and every branch scene on the float64 reference: name -> dict(aligner state before, outs)"""
    out = {}
    for seed, F in SEEDED:
        sc = R.imu_scene(seed, F, samples=3 if F > 11 else 4)
        al = R.Aligner(TIC=tuple(float(t) for t in sc["motion"].tic))
        R.feed(al, sc)
        out[f"seed{seed}-F{F}"] = _solve_and_keep(al, R.BGS0)
    for name in R.BRANCHES:
        sc, params, key, Bgs = R.branch_scene(name)
        al = R.Aligner(**params)
        R.feed(al, sc, key)
        if name == "erase":
            al.erase_through(sc["stamps"][2])
        out[name] = _solve_and_keep(al, Bgs)
        if name == "second":
            out["second-2"] = _solve_and_keep(al, out[name]["Bgs"])
    return out


def _solve_and_keep(al, Bgs):
    blob = _scene_blob(al, Bgs)
    Bout, info = al.solve(Bgs)
    return dict(blob=blob, Bgs=Bout, info=info, frames=[al.record(i) for i in range(len(al.frames))], params=dict(al.P))


def _scene_blob(al, Bgs):
    """the state of an Aligner before a solve, for the stand-alone driver"""
    F = len(al.frames)
    v = [float(F), *al.P["TIC"], *al.P["G"], *np.asarray(Bgs, np.float64).ravel()]
    for i, f in enumerate(al.frames):
        v += [*f["R"], *f["T"]]
        if i == 0 or f["pre"] is None:
            v += [0.0, 0.0]
            continue
        s = f["pre"]["state"]
        v += [1.0, float(len(f["pre"]["samples"])), *s["linearized_acc"], *s["linearized_gyr"], *s["linearized_ba"], *s["linearized_bg"]]
        for dt, a, g in f["pre"]["samples"]:
            v += [dt, *a, *g]
    return np.array(v, np.float64).tobytes()


# ---- band = dense, the numpy route, accuracy in mpmath ----------------------------------------------------------------
def test_band_equals_dense_bit_for_bit(solved):
    n_sys = 0
    for name, sv in solved.items():
        for w, (A, b, x) in enumerate(sv["info"]["systems"]):
            nd = 3 * sv["info"]["frames"]
            xb, pb = R.ldl_band(A, b, nd)
            xd, pd, _ = R.ldl_dense(A, b) if 2 * (nd - 3) >= len(b) else (None, 0.0, None)
            assert (xb is None) == (xd is None), (name, w)
            if xb is not None:
                assert np.array_equal(np.array(xb), np.array(xd), equal_nan=True) and pb == pd, (name, w)
                n_sys += 1
    assert n_sys >= 5 * len(SEEDED)
    print(f"[align ref] band = dense on {n_sys} systems")


def test_accuracy_against_numpy_in_mpmath(solved):
    """the normwise backward error of each of the five solves of every seeded scene, beside numpy.linalg.solve's on the same
    system; the bar is max(10 G, u)"""
    over, rows = [], []
    for seed, F in SEEDED:
        sv = solved[f"seed{seed}-F{F}"]
        assert sv["info"]["reason"] == R.OK, (seed, F)
        for w, (A, b, x) in enumerate(sv["info"]["systems"]):
            if w == R.SYSTEMS - 1:
                x = R.ldl_band(A, b, 3 * F)[0]                 # as it was solved: the kept x has its tail divided by 100
            xn = [float(t) for t in np.linalg.solve(np.array(A), np.array(b))]
            e, g = R.backward_error(A, b, x), R.backward_error(A, b, xn)
            xm = R.solve_mp(A, b) if F <= 11 else None
            fwd = max(abs(p - q) for p, q in zip(x, xm)) / max(abs(q) for q in xm) if xm else float("nan")
            rows.append((seed, F, w, e, g, fwd))
            if e > max(10 * g, U):
                over.append((seed, F, w, e, g))
    for r in rows:
        print("[align accuracy] seed %d F %d system %d: backward %.2e (%.3f u), numpy %.2e, forward %.2e" % (r[0], r[1], r[2], r[3], r[3] / U, r[4], r[5]))
    assert not over, over


def test_numpy_route_gives_the_same_result_and_reason(solved):
    """the same systems solved by numpy.linalg.solve: the same boolean and reason on every scene whose gates have clear margins"""
    names = [f"seed{s}-F{F}" for s, F in SEEDED] + ["F4", "gnorm", "mirror", "zero_samples", "second", "erase", "keys", "neg_refined"]
    aside = []
    for name in names:
        sv = solved[name]
        fr = [dict(R=list(f["R"]), T=list(f["T"]), **({k: (f["pre"][k] if k == "sum_dt" else list(f["pre"][k])) for k in ("sum_dt", "delta_p", "delta_v")}
                                                       if f["pre"] else {})) for f in sv["frames"]]
        la = R.linear_alignment(fr, sv["params"]["TIC"], sv["params"]["G"], "numpy")
        gn = R.norm3([float(t) for t in sv["params"]["G"]])
        margins = [abs(abs(R.norm3(la["g_linear"]) - gn) - 1.0), abs(la["s"]) / max(1.0, abs(la["s"]))]
        if min(margins) < 1e-9:
            aside.append(name)
            continue
        assert la["reason"] == sv["info"]["reason"], (name, la["reason"], sv["info"]["reason"])
        if la["reason"] == R.OK:
            assert abs(la["s"] - sv["info"]["s"]) <= 1e-9 * abs(la["s"]) and np.allclose(la["g"], sv["info"]["g"], rtol=0, atol=1e-8)
    print(f"[align ref] numpy route: {len(names)} scenes, {len(aside)} set aside")
    assert len(aside) == 0


# ---- it does what it is for -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [4, 11, 30])
def test_exact_preintegrations_recover_the_truth(F):
    for seed in (1, 2, 3):
        fr, m = R.exact_frames(seed, F)
        la = R.linear_alignment(fr, m.tic, m.gw)
        assert la["reason"] == R.OK
        g_true = m.R_c0_w @ m.gw
        v0 = m.rot(0.0).T @ m.pos(0.0, 1)                       # the body-frame velocity of the first frame
        errs = (abs(la["s"] - m.s) / m.s, np.abs(np.array(la["g"]) - g_true).max() / 9.8, np.abs(np.array(la["x"][:3]) - v0).max() / max(1.0, np.abs(v0).max()))
        print(f"[align truth] F {F} seed {seed}: s {errs[0]:.2e}, g {errs[1]:.2e}, v0 {errs[2]:.2e}")
        assert max(errs) <= (1e-8 if F == 4 else 1e-11), errs   # the solve's accuracy times the system's condition


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_midpoint_error_shrinks_with_the_sample_rate(seed):
    """with midpoint-integrated samples the recovered scale and gravity are closer to the truth at 400 Hz than at 100 Hz"""
    errs = {}
    for rate, samples in ((100, 10), (400, 40)):
        sc = R.imu_scene(seed, 8, samples=samples)
        m = sc["motion"]
        al = R.Aligner(TIC=tuple(float(t) for t in m.tic))
        R.feed(al, sc)
        _, info = al.solve(np.zeros((11, 3)))
        assert info["reason"] == R.OK
        errs[rate] = (abs(info["s"] - m.s) / m.s, float(np.abs(np.array(info["g"]) - m.R_c0_w @ m.gw).max()), float(np.abs(np.array(info["delta_bg"]) - m.bg).max()))
        print(f"[align midpoint] seed {seed} {rate} Hz: s {errs[rate][0]:.3e}, g {errs[rate][1]:.3e}, delta_bg {errs[rate][2]:.3e}")
    assert all(errs[400][k] < errs[100][k] for k in range(3)), errs


# ---- the branches -----------------------------------------------------------------------------------------------------
def test_branches(solved):
    want = dict(F2=R.SINGULAR, F3=R.SINGULAR, F4=R.OK, gnorm=R.GRAVITY_NORM, mirror=R.NEGATIVE_SCALE, gz=R.OK, nan=R.SINGULAR, second=R.OK, erase=R.OK, keys=R.OK,
                neg_refined=R.NEGATIVE_SCALE_REFINED)
    for name, reason in want.items():
        info = solved[name]["info"]
        assert info["reason"] == reason and info["ok"] == (reason == R.OK), (name, R.REASONS[info["reason"]])
        assert all(np.isfinite(np.r_[info["x"], info["g"], info["s"], info["delta_bg"], np.ravel(solved[name]["Bgs"])])), name
        if reason == R.SINGULAR:
            assert not any(info["x"]) and not any(info["g"])
    nr = solved["neg_refined"]["info"]
    assert nr["systems"][0][2][-1] / 100.0 > 0.01 and nr["s"] < -0.1 and len(nr["x"]) == 3 * 8 + 3     # s < 0 only after the refinement
    assert R.normalized3(solved["gz"]["info"]["g_linear"]) == [0.0, 0.0, 1.0]          # TangentBasis's other branch was taken
    assert R.tangent_basis([0.0, 0.0, 9.8]) == [[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]
    al = R.Aligner()
    assert al.solve(R.BGS0)[1]["reason"] == R.TOO_FEW
    # a second solve: Bgs accumulates and the jacobians are those of the last repropagate
    a, b = solved["second"], solved["second-2"]
    assert np.array_equal(b["Bgs"], a["Bgs"] + np.array(b["info"]["delta_bg"])[None, :].repeat(11, 0))
    assert all(np.array_equal(f["pre"]["linearized_bg"], b["Bgs"][0]) and not f["pre"]["linearized_ba"].any() for f in b["frames"][1:])
    assert np.abs(b["info"]["delta_bg"]).max() < 0.3 * np.abs(a["info"]["delta_bg"]).max()
    assert len(solved["erase"]["frames"]) == 7 and solved["zero_samples"]["frames"][3]["samples"] == 0
    with pytest.raises(R.StateError):
        R.Aligner().erase_through(1.0)


# ---- csrc/lvi_align_math.hpp alone, plain and under the host sanitizers ---------------------------------------------
DRIVER = r"""
// stand-alone driver of csrc/lvi_align_math.hpp: VisualIMUAlignment on one thread
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lvi_align_math.hpp"
using namespace lvi_align_math;
static void put(const double* v, int n) { for (int k = 0; k < n; k++) printf(" %a", v[k]); }
int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    double head[40];      // F, TIC, G, Bgs [33]
    while (fread(head, sizeof(double), 40, f) == 40) {
        const int F = (int)head[0];
        if (F < 2 || F > 256) return 4;
        std::vector<Frame> fr((size_t)F);
        std::vector<pm::State> st((size_t)F);
        std::vector<std::vector<double>> jac((size_t)F, std::vector<double>(225)), smp((size_t)F);
        std::vector<double> lin((size_t)F * 12), work(pm::WORK_DOUBLES);
        std::vector<int> cnt((size_t)F, 0);
        for (int i = 0; i < F; i++) {
            double pose[14];
            if (fread(pose, sizeof(double), 14, f) != 14) return 5;
            for (int k = 0; k < 9; k++) fr[i].R[k] = pose[k];
            for (int k = 0; k < 3; k++) fr[i].T[k] = pose[9 + k];
            fr[i].jacobian = jac[i].data();
            if (pose[12] == 0.) continue;
            cnt[i] = (int)pose[13];
            if (cnt[i] < 0 || cnt[i] > 100000) return 6;
            if (fread(&lin[12 * i], sizeof(double), 12, f) != 12) return 7;
            smp[i].resize((size_t)cnt[i] * 7);
            if (fread(smp[i].data(), sizeof(double), smp[i].size(), f) != smp[i].size()) return 8;
            repropagate(st[i], jac[i].data(), &lin[12 * i], &lin[12 * i + 3], &lin[12 * i + 6], &lin[12 * i + 9], cnt[i], smp[i].data(), work.data());
        }
        auto load = [&](int i) {
            fr[i].pre.sum_dt = st[i].sum_dt;
            for (int k = 0; k < 3; k++) { fr[i].pre.delta_p[k] = st[i].delta_p[k]; fr[i].pre.delta_v[k] = st[i].delta_v[k]; }
            for (int k = 0; k < 4; k++) fr[i].pre.delta_q[k] = st[i].delta_q[k];
        };
        for (int i = 1; i < F; i++) load(i);
        Result r{};
        double Bgs[33], zero[3] = {0., 0., 0.};
        const int gy = gyro_bias(fr.data(), F, r.delta_bg, &r.min_pivot[0]);
        for (int k = 0; k < 33; k++) Bgs[k] = head[7 + k] + r.delta_bg[k % 3];
        for (int i = 1; i < F; i++) {
            repropagate(st[i], jac[i].data(), &lin[12 * i], &lin[12 * i + 3], zero, Bgs, cnt[i], smp[i].data(), work.data());
            load(i);
        }
        const int nd = 3 * F, stride = sys_doubles(nd, NB_LINEAR), n4 = nd + NB_LINEAR;
        std::vector<double> sys((size_t)stride * SYSTEMS, 0.), fw((size_t)BW * nd + 4 * n4), x((size_t)n4, 0.);
        double mp0 = r.min_pivot[0];
        if (gy == OK) linear_alignment(fr.data(), F, head + 1, head + 4, sys.data(), fw.data(), r);
        else { r.reason = SINGULAR; r.n_state = n4; }
        r.min_pivot[0] = mp0;
        const int final_w = (r.reason == OK || r.reason == NEGATIVE_SCALE_REFINED) ? SYSTEMS - 1 : 0;
        if (r.reason != SINGULAR) {
            const double* xs = sys.data() + (size_t)stride * final_w + off_x(nd, final_w ? NB_REFINE : NB_LINEAR);
            for (int k = 0; k < r.n_state; k++) x[k] = xs[k];
        }
        printf("%d %d %d %d", r.reason, r.n_state, r.built, F);
        put(r.delta_bg, 3); put(Bgs, 33); put(&r.s, 1); put(r.g_linear, 3); put(r.g, 3); put(r.min_pivot, 6); put(x.data(), n4);
        for (int i = 1; i < F; i++) {
            put(&st[i].sum_dt, 1); put(st[i].delta_p, 3); put(st[i].delta_q, 4); put(st[i].delta_v, 3); put(st[i].linearized_ba, 3); put(st[i].linearized_bg, 3);
            put(jac[i].data(), 225);
        }
        for (int w = 0; w < r.built; w++) {
            const int nb = w ? NB_REFINE : NB_LINEAR, n = nd + nb;
            const double* S = sys.data() + (size_t)stride * w;
            std::vector<double> A((size_t)n * n), xd((size_t)n, 0.);
            c_expand(nd, nb, S, S + off_bord(nd), A.data());
            put(A.data(), n * n); put(S + off_b(nd, nb), n); put(S + off_x(nd, nb), n);
            // the dense statement of the factorisation on the same system
            double mpd = 0.;
            std::vector<double> Ad(A);
            const bool okd = 2 * (nd - 3) >= n && ldl_dense(n, Ad.data(), S + off_b(nd, nb), xd.data(), &mpd) && all_finite(xd.data(), n);
            if (w == SYSTEMS - 1 && okd) xd[n - 1] = xd[n - 1] / 100.0;
            int same = 1;
            for (int k = 0; k < n; k++) same &= (!okd && S[off_x(nd, nb) + k] == 0.) || (okd && xd[k] == S[off_x(nd, nb) + k]);
            printf(" %d", same);
        }
        double lx[6], gz[3] = {0., 0., 9.8};
        tangent_basis(gz, lx);
        put(lx, 6);
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
    d = tmp_path_factory.mktemp("align_header")
    return {"plain": _build_driver(pkg, d / "plain", []),
            "san": _build_driver(pkg, d / "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])}


@pytest.mark.parametrize("which", ["plain", "san"])
def test_math_header_equals_the_float64_reference_bit_for_bit(drivers, solved, tmp_path, which):
    """only IEEE + - * / sqrt in a stated order with contraction off: no tolerance; the sanitizer build must exit clean"""
    names = list(solved)
    (tmp_path / "s.bin").write_bytes(b"".join(solved[k]["blob"] for k in names))
    out = subprocess.run([drivers[which], str(tmp_path / "s.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l.split() for l in out.stdout.split("\n") if l]
    assert len(lines) == len(names)
    for name, line in zip(names, lines):
        sv = solved[name]
        reason, n_state, built, F = (int(t) for t in line[:4])
        v = np.array([float.fromhex(t) if t.startswith(("0x", "-0x", "nan", "-nan", "inf", "-inf")) else float(t) for t in line[4:]])
        n4, at = 3 * F + 4, 0

        def take(n):
            nonlocal at
            at += n
            return v[at - n:at]
        delta_bg, Bgs, s, g_linear, g, min_pivot, x = take(3), take(33), take(1)[0], take(3), take(3), take(6), take(n4)
        frames = [sv["frames"][0]]
        for i in range(1, F):
            want = sv["frames"][i]
            pre = dict(sum_dt=take(1)[0], delta_p=take(3), delta_q=take(4), delta_v=take(3), linearized_ba=take(3), linearized_bg=take(3),
                       linearized_acc=want["pre"]["linearized_acc"], linearized_gyr=want["pre"]["linearized_gyr"], jacobian=None)
            pre["jacobian"] = take(225).reshape(15, 15)
            frames.append(dict(want, pre=pre))
        systems = []
        for w in range(built):
            n = 3 * F + (4 if w == 0 else 3)
            systems.append((take(n * n).reshape(n, n), take(n), take(n)))
            assert take(1)[0] == 1.0, (name, w, "band != dense in the header")
        assert np.array_equal(take(6), np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])) and at == len(v)
        R.check_solve(f"{which}:{name}", sv, reason, n_state, built, delta_bg, Bgs, s, g_linear, g, min_pivot, x, frames, systems)
    print(f"[align header] {which}: {len(names)} solves equal the float64 reference bit for bit")


def test_excitation_reference():
    sc = R.imu_scene(5, 6)
    al = R.Aligner()
    R.feed(al, sc)
    v = al.excitation()
    tg = np.array([np.array(al.frames[i]["pre"]["state"]["delta_v"]) / al.frames[i]["pre"]["state"]["sum_dt"] for i in range(1, 6)])
    assert abs(v - np.sqrt(((tg - tg.mean(0)) ** 2).sum() / 5)) <= 1e-12 * v and v > 0


# ---- the tail of visualInitialAlign -----------------------------------------------------------------------------------
def _apply_case(seed, opposite):
    rs = np.random.RandomState(seed)
    m = R.Motion(seed)
    fc = 10
    poses = [m.pose(0.1 * i) for i in range(fc + 1)]
    Ps, Rs = np.array([p[1] for p in poses]), np.array([p[0] for p in poses])
    keys = [i for i in range(14) if i % 4 != 1][:fc + 1]
    key_R = np.array([m.pose(0.07 * i)[0].ravel() for i in keys])
    x = np.r_[rs.normal(0, 1, 3 * 14 + 2), m.s]
    g = np.array([0.0, 0.0, -9.8]) if opposite else m.R_c0_w @ m.gw
    return dict(fc=fc, TIC=m.tic, Ps=Ps, Rs=Rs, x=x, g=g, key_R=key_R)


def _apply_lib(pkg, lib, c):
    P = pkg.align
    d = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    p = P.AlignParams()
    lib.dll.lvi_align_params_default(ctypes.byref(p))
    p.TIC = (ctypes.c_double * 3)(*c["TIC"])
    Ps, Rs, g, Vs, rot, flags = c["Ps"].copy(), c["Rs"].reshape(-1, 9).copy(), c["g"].copy(), np.zeros((c["fc"] + 1, 3)), np.zeros(9), ctypes.c_int32(0)
    x, key_R = np.ascontiguousarray(c["x"]), np.ascontiguousarray(c["key_R"])
    lib.check(lib.dll.lvi_align_apply(ctypes.byref(p), c["fc"], d(Ps), d(Rs), d(Vs), d(x), len(x), d(g), d(key_R), len(key_R), d(rot), ctypes.byref(flags)),
              "lvi_align_apply")
    return list(Ps.ravel()) + list(Rs.ravel()) + list(Vs.ravel()) + list(g) + list(rot), flags.value


def _check_apply(c, got, what):
    """against the mpmath statement at max(10 G, 16 ulp of the largest entry); G: the float64-numpy route's distance"""
    vals, flags = got
    mp = R.apply(c["fc"], c["TIC"], c["Ps"], c["Rs"], c["x"], c["g"], c["key_R"], R._MPX)
    route = R.apply(c["fc"], c["TIC"], c["Ps"], c["Rs"], c["x"], c["g"], c["key_R"], R._NPX)
    ref = R.apply_flat(mp)
    G = max(abs(mpmath.mpf(float(a)) - b) for a, b in zip(R.apply_flat(route), ref))
    big = max(abs(float(t)) for t in ref)
    bar = max(10 * float(G), 16 * 2.0 ** -52 * big)
    err = max(abs(mpmath.mpf(float(a)) - b) for a, b in zip(vals, ref))
    print(f"[align apply] {what}: error {float(err):.3e}, numpy route {float(G):.3e}, bar {bar:.3e}")
    assert len(vals) == len(ref) and float(err) <= bar and flags == mp[5]
    return mp


@pytest.mark.parametrize("opposite", [False, True])
def test_apply_reference_against_mpmath(opposite):
    c = _apply_case(11, opposite)
    f = R.apply(c["fc"], c["TIC"], c["Ps"], c["Rs"], c["x"], c["g"], c["key_R"])
    mp = _check_apply(c, (R.apply_flat(f), f[5]), "float64 reference")
    Ps, Rs, Vs, g, rot, flags = mp
    assert flags == (R.APPLY_OPPOSITE if opposite else 0)
    assert abs(g[0]) < 1e-30 and abs(g[1]) < 1e-30 and abs(g[2] - mpmath.mpf(9.8)) < 1e-14        # gravity along +z
    assert abs(mpmath.atan2(Rs[0][3], Rs[0][0])) < 1e-30 and all(abs(t) < 1e-30 for t in Ps[0])   # no yaw in frame 0, which sits at the origin
    # the kv walk: Vs[kv] comes from the kv-th key frame of the list, not from list index kv
    assert all(abs(a - b) < 1e-25 for a, b in zip(Vs[3], R.PR.mat3_vec(rot, R.PR.mat3_vec([mpmath.mpf(float(t)) for t in c["key_R"][3]],
                                                                                           [mpmath.mpf(float(t)) for t in c["x"][9:12]]))))
