"""CPU tier of the sliding-window solve (include/lvi_win.h): the ABI checks, load_window_yaml, the reference
tests/win_ref.py against central differences on the manifold, csrc/lvi_imu_math.hpp compiled alone (plain and as a
stand-alone program under the host sanitizers) against the reference, and the conditions the GPU tier's scenes rely on."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import marg_ref as M
import win_ref as R
import win_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.2e-16


def _header():
    return open(os.path.join(ROOT, "include", "lvi_win.h")).read()


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(lvi_win_[a-z0-9_]+)\s*\(", txt)))


# ---- ABI -------------------------------------------------------------------------------------------
def test_header_and_win_binding_agree(pkg):
    W = pkg.win
    assert _declared() == sorted(W.WIN_SIGNATURES.keys())
    assert len(_declared()) == 15
    assert not set(_declared()) & set(pkg._abi.SIGNATURES) and not set(_declared()) & set(pkg.marg.MARG_SIGNATURES)
    txt = _header()
    for name, val in (("ABI_VERSION", 1), ("MAX_BLOCKS", W.MAX_BLOCKS), ("MAX_PROJECTIONS", W.MAX_PROJECTIONS), ("MAX_ELIMINATED", W.MAX_ELIMINATED),
                      ("MAX_IMU", W.MAX_IMU), ("MAX_PRIOR_ROWS", W.MAX_PRIOR_ROWS), ("MAX_DIM", W.MAX_DIM), ("MAX_BLOCK_SIZE", W.MAX_BLOCK_SIZE),
                      ("MAX_ITERATIONS", W.MAX_ITERATIONS), ("SHARE", W.SHARE), ("CHOL_BLOCK", W.CHOL_BLOCK), ("CONSTANT", W.CONSTANT), ("ELIMINATED", W.ELIMINATED),
                      ("NOT_FINITE", W.NOT_FINITE), ("BAD_COVARIANCE", W.BAD_COVARIANCE), ("TERM_FUNCTION", W.TERM_FUNCTION), ("TERM_GRADIENT", W.TERM_GRADIENT), ("TERM_PARAMETER", W.TERM_PARAMETER),
                      ("TERM_ITERATIONS", W.TERM_ITERATIONS), ("TERM_TIME", W.TERM_TIME), ("TERM_RADIUS", W.TERM_RADIUS), ("TERM_INVALID_STEPS", W.TERM_INVALID_STEPS),
                      ("STEP_GAUSS_NEWTON", W.STEP_GAUSS_NEWTON), ("STEP_CAUCHY", W.STEP_CAUCHY), ("STEP_INTERPOLATED", W.STEP_INTERPOLATED)):
        assert int(re.search(r"#define LVI_WIN_%s\s+(\d+)" % name, txt).group(1)) == val, name
    # the capacities the issue asks for: 16 frames, 8192 projections, 2048 eliminated blocks, a prior of 256 rows
    assert W.MAX_DIM >= 16 * 15 + 7 and W.MAX_PROJECTIONS >= 8192 and W.MAX_ELIMINATED >= 2048 and W.MAX_PRIOR_ROWS >= 256 and W.MAX_IMU >= 15 and W.MAX_ITERATIONS == 64
    assert (W.SHARE, W.CHOL_BLOCK) == (R.SHARE, R.CHOL_BLOCK) and (W.CONSTANT, W.ELIMINATED) == (R.CONSTANT, R.ELIMINATED)
    assert (W.TERM_FUNCTION, W.TERM_GRADIENT, W.TERM_PARAMETER, W.TERM_ITERATIONS, W.TERM_RADIUS, W.TERM_INVALID_STEPS) == \
        (R.TERM_FUNCTION, R.TERM_GRADIENT, R.TERM_PARAMETER, R.TERM_ITERATIONS, R.TERM_RADIUS, R.TERM_INVALID_STEPS)
    assert all(s in txt for s in ("estimator.cpp:696-811", ":792-805", "imu_factor.h:18-178", "integration_base.h:160-186", ":332-380",
                                  "pose_local_parameterization.cpp:3-19", ":735-744", ":719-726", "restated from recall"))
    assert '#include "lvi_marg.h"' in txt and "typedef struct lvi_marg_projection" not in txt       # the record is included, not copied
    assert "lvi_win" not in open(os.path.join(ROOT, "include", "lvi_hotpath.h")).read()
    assert "lvi_win" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lvi_marg.h")).read(), flags=re.S)


def test_record_layouts(pkg):
    W = pkg.win
    txt = _header()
    for cname, cls, size in (("lvi_win_caps", W.WinCaps, 24), ("lvi_win_params", W.WinParams, 200), ("lvi_win_imu", W.WinImu, 3752), ("lvi_win_info", W.WinInfo, 64),
                             ("lvi_win_iteration", W.WinIteration, 96)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in re.findall(r"\b(?:int32_t|double)\s+([^;]+);", body) for n in re.findall(r"([A-Za-z_][A-Za-z_0-9]*)(?:\[\d+\])?\s*(?:,|$)", decl)]
        assert names == [f[0] for f in cls._fields_], cname
        assert ctypes.sizeof(cls) == size, cname
    assert W.IMU_DTYPE.itemsize == 3752 and list(W.IMU_DTYPE.names) == [f[0] for f in W.WinImu._fields_]
    assert [W.IMU_DTYPE.fields[n][1] for n in W.IMU_DTYPE.names] == [getattr(W.WinImu, n).offset for n in W.IMU_DTYPE.names]
    # every constant of the loop is a parameter
    assert set(R.DEFAULTS) == {f[0] for f in W.WinParams._fields_}


def test_hip_library_exports_the_win_abi_and_the_oracle_does_not(pkg, oracle):
    dll = ctypes.CDLL(pkg.HIP_LIB_PATH)
    for name in _declared():
        assert hasattr(dll, name), f"{name} missing from liblvi_hip.so"
    lib = pkg.win.bind(pkg.load_hip())
    assert lib.dll.lvi_win_abi_version() == 1 and lib.dll.lvi_marg_abi_version() == 1 and lib.dll.lvi_abi_version() == 6
    p = pkg.win.WinParams()
    lib.dll.lvi_win_params_default(ctypes.byref(p))
    for k, v in R.DEFAULTS.items():
        got = getattr(p, k)
        assert (tuple(got) if k == "G" else got) == v, k
    syms = subprocess.run(["nm", "-D", "--defined-only", oracle.path], capture_output=True, text=True).stdout
    assert "lvi_abi_version" in syms and "lvi_win_" not in syms
    # the accessor into the marginaliser's handle is not exported
    syms = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    assert "marg_prior_view" not in syms


def test_window_solver_fails_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.LviError) as e:
        pkg.WindowSolver(pkg.load_hip(), max_blocks=8, max_projections=8, max_dim=8)
    assert e.value.code == pkg._abi.LVI_ERR_NO_DEVICE


def test_load_window_yaml(pkg, tmp_path):
    p = tmp_path / "params_camera.yaml"
    p.write_text("%YAML:1.0\n---\nmax_solver_time: 0.035\nmax_num_iterations: 10\nestimate_extrinsic: 0\nestimate_td: 1\nacc_n: 0.02\ngyr_n: 0.01\n"
                 "acc_w: 0.002\ngyr_w: 4.0e-5\ng_norm: 9.805\nimage_height: 480\ntd: 0.0\n")
    c = pkg.config.load_window_yaml(str(p))
    assert c == dict(max_solver_time=0.035, max_num_iterations=10, estimate_extrinsic=0, estimate_td=True, acc_n=0.02, gyr_n=0.01, acc_w=0.002, gyr_w=4.0e-5,
                     g_norm=9.805, G=[0.0, 0.0, 9.805])


# ---- the reference itself ---------------------------------------------------------------------------
def _imu_cases(dbg_scale):
    """(pose_i, speed_bias_i, pose_j, speed_bias_j, preintegration) of seeded scenes, the state perturbed; dbg_scale 0 keeps
    Bgi at linearized_bg"""
    out = []
    for seed in (31, 32, 33):
        sc = S.make_scene(seed, 3, [3] * 2)
        blocks = {op[1]: np.array(op[2], np.float64) for op in sc["ops"] if op[0] == "block"}
        for op in sc["ops"]:
            if op[0] == "imu":
                rec = op[1]
                sb_i = blocks[rec["speed_bias_i"]].copy()
                sb_i[6:9] = rec["linearized_bg"] + dbg_scale * np.random.RandomState(seed).normal(0, 1e-3, 3)
                out.append((blocks[rec["pose_i"]], sb_i, blocks[rec["pose_j"]], blocks[rec["speed_bias_j"]], rec))
    return out


def _perturbed(args, block, k, h):
    a = [np.array(v, np.float64) for v in args]
    if len(a[block]) == 7:
        d = np.zeros(6)
        d[k] = h
        a[block] = R.pose_plus(a[block], d, R.F64)
    else:
        a[block][k] += h
    return a


H_CD = 1e-6


@pytest.mark.parametrize("dbg_scale", [0.0, 1.0])
def test_imu_jacobians_equal_central_differences_on_the_manifold(dbg_scale):
    """The raw factor (before sqrt_info, which is a constant matrix): central differences with h = 1e-6 over Plus.  Bound:
    rounding 2 u s / 2h and truncation h^2 s / 6 with s the scale of the residual's arguments (|P|, |V| sum_dt, G sum_dt^2 and
    the preintegration, all below 10 here, the third derivatives of a rotation being of that size too), times 10; and, where
    Bgi is not linearized_bg, what the reference's own formulas leave out: the bg column is taken at delta_q and not at
    corrected_delta_q (:124) and corrected_delta_q is not unit (:96, :150), both of relative size |theta| = |dq_dbg dbg|."""
    G = (0.0, 0.0, 9.8)
    worst = 0.0
    for case in _imu_cases(dbg_scale):
        args, rec = case[:4], case[4]
        r, J = R.imu_eval_raw(*args, rec, G, R.F64)
        theta = np.linalg.norm(rec["jacobian"][3:6, 12:15] @ (args[1][6:9] - rec["linearized_bg"]))
        scale = 10.0
        bound = 10 * (2 * U * scale / (2 * H_CD) + H_CD ** 2 * scale / 6) + 2 * theta * np.abs(J).max()
        col = 0
        for b, ls in enumerate((6, 9, 6, 9)):
            for k in range(ls):
                rp, _ = R.imu_eval_raw(*_perturbed(args, b, k, H_CD), rec, G, R.F64, jac=False)
                rm, _ = R.imu_eval_raw(*_perturbed(args, b, k, -H_CD), rec, G, R.F64, jac=False)
                worst = max(worst, np.abs((rp - rm) / (2 * H_CD) - J[:, col + k]).max() / bound)
            col += ls
    print(f"[win ref] dbg x {dbg_scale}: analytic vs central differences, worst gap / bound {worst:.3e}")
    assert worst <= 1.0


def test_sqrt_info_is_the_upper_factor_of_the_information():
    for case in _imu_cases(0.0)[:2]:
        cov = case[4]["covariance"]
        Sm = R.imu_sqrt_info(cov, R.MP)
        E = Sm.T @ Sm @ R.MP.arr(cov) - R.MP.arr(np.eye(15))
        gap = float(max(abs(v) for v in E.ravel()))
        Sf = R.imu_sqrt_info(cov, R.F64)
        rel = M.gap(Sf, Sm) / float(max(abs(v) for v in Sm.ravel()))
        print(f"[win ref] sqrt_info' sqrt_info covariance - I in mpmath {gap:.3e}; float64 vs mpmath relative {rel:.3e}; cond {np.linalg.cond(cov):.3e}")
        assert gap < 1e-30 and np.allclose(np.tril(Sf, -1), 0.0)
        assert rel <= 100 * U * np.linalg.cond(cov)


# ---- csrc/lvi_imu_math.hpp alone, plain and under the host sanitizers ------------------------------------------
DRIVER = r"""
// stand-alone driver of csrc/lvi_imu_math.hpp: the IMU factor as the kernels call it, run on the host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "lvi_imu_math.hpp"
using namespace lvi_imu_math;
static void put(const double* v, int n) { for (int i = 0; i < n; i++) printf("%a ", v[i]); printf("\n"); }
int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 3;
    if (!strcmp(argv[1], "imu")) {
        std::vector<double> in(502);
        while (fread(in.data(), sizeof(double), in.size(), f) == in.size()) {
            const double *pi = &in[0], *si = &in[7], *pj = &in[16], *sj = &in[23], *G = &in[32];
            ImuPre p;
            p.sum_dt = in[35];
            memcpy(p.delta_p, &in[36], 24); memcpy(p.delta_q, &in[39], 32); memcpy(p.delta_v, &in[43], 24);
            memcpy(p.linearized_ba, &in[46], 24); memcpy(p.linearized_bg, &in[49], 24); memcpy(p.jacobian, &in[52], 225 * 8);
            std::vector<double> S(225), work(675), r(15), J(450), out(15 + 450);
            if (!imu_sqrt_info(&in[277], S.data(), work.data())) return 4;
            imu_eval_raw(pi, si, pj, sj, p, G, r.data(), J.data());
            for (int i = 0; i < 15; i++) {
                out[i] = imu_info_dot(S.data(), i, r.data(), 1, 0);
                for (int c = 0; c < 30; c++) out[15 + 30 * i + c] = imu_info_dot(S.data(), i, J.data(), 30, c);
            }
            put(out.data(), 465);
            put(S.data(), 225);
            imu_eval_raw(pi, si, pj, sj, p, G, r.data(), nullptr);
            put(r.data(), 15);
        }
    } else if (!strcmp(argv[1], "plus")) {
        double in[13], o[7];
        while (fread(in, sizeof(double), 13, f) == 13) { pose_plus(in, in + 7, o); put(o, 7); }
    } else if (!strcmp(argv[1], "notspd")) {
        std::vector<double> c(225, 0.), S(225), work(675);
        for (int i = 0; i < 15; i++) c[16 * i] = i == 7 ? -1. : 1.;
        return imu_sqrt_info(c.data(), S.data(), work.data()) ? 5 : 0;
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
    d = tmp_path_factory.mktemp("imu_header")
    return {"plain": _build_driver(pkg, d / "plain", []),
            "san": _build_driver(pkg, d / "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])}


def _run(exe, mode, path):
    r = subprocess.run([exe, mode, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return [np.array([float.fromhex(x) for x in l.split()]) for l in r.stdout.split("\n") if l]


@pytest.mark.parametrize("which", ["plain", "san"])
def test_math_header_imu_factor_equals_the_reference(drivers, tmp_path, which):
    """Bound per case and quantity: max(10 G, floor), G the float64-to-mpmath distance of the reference for that case; floor
    = 15 u x the largest entry (a 15-term product sum).  The factorisation of a covariance of condition 1e9 and more is
    where G comes from."""
    G3 = np.array([0.0, 0.0, 9.8])
    cases = _imu_cases(1.0)[:4]
    blob = b""
    for pi, si, pj, sj, rec in cases:
        blob += np.r_[pi, si, pj, sj, G3, rec["sum_dt"], rec["delta_p"], rec["delta_q"], rec["delta_v"], rec["linearized_ba"], rec["linearized_bg"],
                      rec["jacobian"].ravel(), rec["covariance"].ravel()].astype(np.float64).tobytes()
    (tmp_path / "i.bin").write_bytes(blob)
    got = _run(drivers[which], "imu", tmp_path / "i.bin")
    assert len(got) == 3 * len(cases)
    worst = 0.0
    for k, (pi, si, pj, sj, rec) in enumerate(cases):
        ref = []
        for X in (R.F64, R.MP):
            Sq = R.imu_sqrt_info(rec["covariance"], X)
            r, J = R.imu_factor(pi, si, pj, sj, rec, G3, X, Sq)
            raw, _ = R.imu_eval_raw(pi, si, pj, sj, rec, G3, X, jac=False)
            ref.append((np.concatenate([r, J.ravel()]), Sq.ravel(), raw))
        for g, wf, wm in zip(got[3 * k:3 * k + 3], ref[0], ref[1]):
            Gd = M.gap(wf, wm)
            tol = max(10 * Gd, 15 * U * float(np.abs(wf).max()))
            err = float(np.abs(g - wf).max())
            worst = max(worst, err / tol)
            assert err <= tol, (k, err, tol)
    print(f"[imu header] {which}: residual, Jacobians and sqrt_info vs reference, worst error / bound {worst:.3e}")
    assert _run(drivers[which], "notspd", tmp_path / "i.bin") == []


@pytest.mark.parametrize("which", ["plain", "san"])
def test_math_header_pose_plus_equals_the_reference(drivers, tmp_path, which):
    rs = np.random.RandomState(5)
    cases = [(np.r_[rs.normal(0, 1, 3), M.rand_quat(rs, 1.0)], rs.normal(0, 10 ** -k, 6)) for k in range(1, 7)]
    (tmp_path / "p.bin").write_bytes(b"".join(np.r_[x, d].tobytes() for x, d in cases))
    got = _run(drivers[which], "plus", tmp_path / "p.bin")
    worst = max(np.abs(g - R.pose_plus(x, d, R.F64)).max() for g, (x, d) in zip(got, cases))
    print(f"[imu header] {which}: Plus vs reference {worst:.3e}")
    assert len(got) == 6 and worst <= 8 * U * 3 and all(abs(np.linalg.norm(g[3:]) - 1) <= 4 * U for g in got)


# ---- the conditions of the GPU tier's scenes ----------------------------------------------------------------
def test_scene_shapes():
    want = dict(two_frames=(37, 6), three_td=(52, 8), three_plain=(45, 8), all_constant=(52, 0), half_constant=(52, 3), eleven_frames=(172, 6), chol_32=(32, 6),
                chol_33=(33, 6), chol_64=(64, 8), chol_65=(65, 8))
    for name, shape in want.items():
        p = S.problem(name, R.F64)
        assert p.layout()[2:] == shape, name
    for name, n in (("share", R.SHARE), ("share_plus_1", R.SHARE + 1), ("two_shares_plus_1", 2 * R.SHARE + 1)):
        assert len(S.problem(name, R.F64).proj) == n
    p = S.problem("eleven_frames", R.F64)
    per = [sum(1 for r in p.proj if r["feature"] == M.ID_FEATURE + k) for k in range(6)]
    assert per[0] == 10 and per[1] == 1                                # seen in all 11 frames; a single factor
    assert len(S.problem("skipped_imu", R.F64).imu) == 1 and S.problem("no_prior", R.F64).prior is None


def test_shared_front_scene_is_one_system_in_both_references():
    """the scene of tests/test_gpu_win.py's comparison of the two handles: both references take it, its shapes are the ones
    meant, and the permutation worked out from the two layout rules carries the marginaliser's A, b onto the window's H, g.
    Both references add the factors' blocks up in factor order, so the float64 sums are the same numbers."""
    blocks, recs = S.shared_front_scene()
    perm = S.shared_front_permutation(blocks, recs)
    mg, pr = M.Marg(M.F64), R.Problem(R.F64)
    for b, v in blocks:
        mg.set_block(b, v)
        pr.set_block(b, v, 0)
    for rec in recs:
        mg.add_projection(rec)
        pr.add_projection(rec)
    A, b, m, n = mg.system()
    sys = pr.system(pr.x0())
    assert len(recs) == R.SHARE + 1 == M.SHARE + 1 and (m, n) == (135, 19) and (sys["D"], sys["E"]) == (154, 0)
    assert sorted(perm) == list(range(154)) and list(perm[:6]) == list(range(6)) and perm[6] == 135 and perm[18 + 6 + 1] == 6
    assert np.array_equal(M.to_f64(A)[np.ix_(perm, perm)], M.to_f64(sys["H"])) and np.array_equal(M.to_f64(b)[perm], M.to_f64(sys["g"]))
    assert mg.marginalize()["rank"] > 0


def test_the_three_radii_give_the_three_step_kinds():
    kinds = [R.solve(S.problem("two_frames", R.F64, initial_radius=rad, max_iterations=1))["log"][1]["step_kind"] for rad in S.STEP_RADII]
    assert kinds == [R.STEP_GAUSS_NEWTON, R.STEP_INTERPOLATED, R.STEP_CAUCHY]


def test_decision_scenes_take_the_same_decisions_in_float64_and_mpmath():
    """Every scene of S.SOLVE_SCENES the GPU tier compares decision by decision: float64 and mpmath decide alike and every
    margin is at least 1000 x the distance between the two arithmetics of the quantity decided.  A scene that fails this is
    named here and compared on systems and single steps only (S.admitted())."""
    admitted = S.admitted()
    for name in S.SOLVE_SCENES:
        f, m = S.solve_reference(name)
        same = R.decisions(f) == R.decisions(m)
        ratio, where = R.min_margin(f, m) if same else (0.0, "the sequences differ")
        print(f"[win ref] {name}: iterations {f['iterations']} termination {f['termination']} same decisions {same}; smallest margin / distance {ratio:.3e} ({where})"
              f"; {'admitted' if name in admitted else 'systems and single steps only'}")
        assert (name in admitted) == (same and ratio >= 1000.0)
    assert admitted == S.SOLVE_SCENES, "a scene left the decision-sequence comparison"


def test_rejected_step_scene():
    """`no_prior` within 10 iterations holds a rejected step in both arithmetics: the GPU tier's single-step test relies on it"""
    f, m = S.solve_reference("no_prior", max_iterations=10)
    rej = [e["iteration"] for e in f["log"][1:] if not e["accepted"]]
    assert rej and R.decisions(f) == R.decisions(m), (rej, R.decisions(f), R.decisions(m))
    ratio, where = R.min_margin(f, m)
    print(f"[win ref] no_prior, 10 iterations: decisions {R.decisions(f)[0]}; smallest margin / distance {ratio:.3e} ({where})")
    assert ratio >= 1000.0


def test_mu_retry_scene_is_an_exact_underflow_in_float64():
    """`chol_33` with min_diagonal 1e-30 and mu 1e-300: the pivot of the free block no factor names is mu x 1e-30, which is zero
    in float64 until mu reaches 1e-293 (seven retries) whatever the order of the sums, since nothing else enters that pivot.  In
    exact arithmetic S is positive definite for every mu > 0, so mpmath never retries: a retry exists in float64 only, and
    the GPU tier compares the count and the final mu with float64 and the step with both at that final mu."""
    f = R.solve(S.problem("chol_33", R.F64, max_iterations=1, **S.RETRY_PARAMS))
    m = R.solve(S.problem("chol_33", R.MP, max_iterations=1, **S.RETRY_PARAMS))
    e = f["log"][1]
    piv = [float(v) for n, v, _ in e["margins"] if n == "pivot"]
    assert e["mu_retries"] == 7 and piv[:7] == [0.0] * 7 and piv[7] > 0 and 0.99e-293 < e["mu"] < 1.01e-293 and e["accepted"] == 1
    assert m["log"][1]["mu_retries"] == 0


def test_host_libraries_link_with_and_without_the_window_solve(pkg, oracle, tmp_path):
    """the oracle-linked host library builds without the window flattening; the HIP one exports it"""
    H = pkg.host_api
    out = tmp_path / "liblvi_host_oracle.so"
    H.build_host_library(str(out), os.path.dirname(oracle.path), "lvi_oracle", extra=("-fopenmp",))
    assert not H.HostLibrary(str(out)).has_win
    assert "lvh_win_" not in subprocess.run(["nm", "-D", "--defined-only", str(out)], capture_output=True, text=True).stdout
    assert os.path.exists(H.HOST_HIP_LIB), "host/liblvi_host_hip.so not built: run __graft_entry__.build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", H.HOST_HIP_LIB], capture_output=True, text=True).stdout
    for name in ("lvh_win_create", "lvh_win_destroy", "lvh_win_handle", "lvh_win_set_imu", "lvh_win_set_lidar_flags", "lvh_win_optimize", "lvh_win_get_window",
                 "lvh_win_last_error"):
        assert re.search(r"\b%s\b" % name, syms), name
    assert H.HostLibrary(H.HOST_HIP_LIB).has_win and H.COMPONENTS["win"].sources == ("lvi_win_capi.cpp",)
    assert H.COMPONENTS["marg"].sources == ("lvi_marg_capi.cpp",) and H.component_sources(["win"]) == ("lvi_marg_capi.cpp", "lvi_win_capi.cpp")
