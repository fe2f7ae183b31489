"""CPU tier of the sliding-window marginalisation (include/lvi_marg.h): the ABI / host-library link checks, the
reference tests/marg_ref.py against central differences, csrc/lvi_marg_math.hpp compiled alone (plain and under the host
sanitizers) against the reference, the host helpers of csrc/lvi_winsys.hpp in the same driver, and the conditions of the GPU
tier's scenes."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import marg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Central differences with h = 1e-6 on a residual scaled by sqrt_info = 306.7 whose arguments are O(1) and whose depth is
# >= 4: rounding 2 x 2.2e-16 x |r| / 2h with |r| <= 306.7 x 2 gives 1.4e-7; truncation h^2 / 6 x |r'''| with third
# derivatives up to 306.7 x 1e2 gives 5e-9.  Bound: 10 x their sum.
H_CD = 1e-6
JAC_GAP_BOUND = 10 * (2 * 2.2e-16 * 2 * R.SQRT_INFO / (2 * H_CD) + H_CD ** 2 / 6 * R.SQRT_INFO * 1e2)
# the header against the float64 reference: both evaluate the same formulas in double in another order; entries reach
# 306.7 x 10 and pass through ~30 operations
HEADER_TOL = 30 * 2.2e-16 * R.SQRT_INFO * 10


def _declared():
    txt = open(os.path.join(ROOT, "include", "lvi_marg.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lvi_marg_[a-z0-9_]+)\s*\(", txt)))


# ---- ABI -------------------------------------------------------------------------------------------
def test_header_and_marg_binding_agree(pkg):
    M = pkg.marg
    assert _declared() == sorted(M.MARG_SIGNATURES.keys())
    assert len(_declared()) == 16
    assert not set(_declared()) & set(pkg._abi.SIGNATURES), "the marg ABI must stay out of lvi_hotpath.h's table"
    txt = open(os.path.join(ROOT, "include", "lvi_marg.h")).read()
    for name, val in (("ABI_VERSION", 1), ("MAX_BLOCKS", M.MAX_BLOCKS), ("MAX_PROJECTIONS", M.MAX_PROJECTIONS), ("MAX_DENSE_FACTORS", M.MAX_DENSE_FACTORS),
                      ("MAX_DENSE_ROWS", M.MAX_DENSE_ROWS), ("MAX_DROP_DIM", M.MAX_DROP_DIM), ("MAX_KEEP_DIM", M.MAX_KEEP_DIM), ("MAX_BLOCK_SIZE", M.MAX_BLOCK_SIZE),
                      ("MAX_SWEEPS", M.MAX_SWEEPS), ("SHARE", M.SHARE), ("LOSS_NONE", M.LOSS_NONE), ("LOSS_CAUCHY", M.LOSS_CAUCHY), ("LOSS_HUBER", M.LOSS_HUBER),
                      ("EIG_NOT_CONVERGED", M.EIG_NOT_CONVERGED), ("NOT_FINITE", M.NOT_FINITE)):
        assert int(re.search(r"#define LVI_MARG_%s\s+(\d+)" % name, txt).group(1)) == val, name
    assert M.SHARE == R.SHARE and (M.LOSS_NONE, M.LOSS_CAUCHY, M.LOSS_HUBER) == (R.LOSS_NONE, R.LOSS_CAUCHY, R.LOSS_HUBER)
    # the declarations cite the reference lines they replace, and the header states the permutation
    assert all(s in txt for s in (":174-296", ":298-318", ":332-380", ":37-68", "estimator.cpp:813-976", ":877, :885", ":837-844", ":896-913", ":946-973"))
    assert "column permutation" in txt and "keep_block_idx" in txt
    assert "lvi_marg" not in open(os.path.join(ROOT, "include", "lvi_hotpath.h")).read()


def test_record_layouts(pkg):
    M = pkg.marg
    txt = open(os.path.join(ROOT, "include", "lvi_marg.h")).read()
    for cname, cls, size in (("lvi_marg_caps", M.MargCaps, 24), ("lvi_marg_params", M.MargParams, 48), ("lvi_marg_projection", M.MargProjection, 136),
                             ("lvi_marg_info", M.MargInfo, 56)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in re.findall(r"\b(?:int32_t|double)\s+([^;]+);", body) for n in re.findall(r"([A-Za-z_][A-Za-z_0-9]*)(?:\[\d+\])?\s*(?:,|$)", decl)]
        assert names == [f[0] for f in cls._fields_], cname
        assert ctypes.sizeof(cls) == size
    assert M.PROJECTION_DTYPE.itemsize == 136 and list(M.PROJECTION_DTYPE.names) == [f[0] for f in M.MargProjection._fields_]
    assert [M.PROJECTION_DTYPE.fields[n][1] for n in M.PROJECTION_DTYPE.names] == [getattr(M.MargProjection, n).offset for n in M.PROJECTION_DTYPE.names]


def test_hip_library_exports_the_marg_abi_and_the_oracle_does_not(pkg, oracle):
    dll = ctypes.CDLL(pkg.HIP_LIB_PATH)
    for name in _declared():
        assert hasattr(dll, name), f"{name} missing from liblvi_hip.so"
    lib = pkg.marg.bind(pkg.load_hip())
    assert lib.dll.lvi_marg_abi_version() == 1
    assert lib.dll.lvi_abi_version() == 6
    p = pkg.marg.MargParams()
    lib.dll.lvi_marg_params_default(ctypes.byref(p))
    assert (p.loss_type, p.max_sweeps, p.loss_a, p.sqrt_info, p.tr_over_row, p.half_row, p.eps) == (R.LOSS_CAUCHY, 30, 1.0, R.SQRT_INFO, 0.0, 240.0, R.EPS)
    syms = subprocess.run(["nm", "-D", "--defined-only", oracle.path], capture_output=True, text=True).stdout
    assert "lvi_abi_version" in syms and "lvi_marg_" not in syms


def test_marginalizer_fails_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.LviError) as e:
        pkg.Marginalizer(pkg.load_hip(), max_blocks=8, max_projections=8, max_drop_dim=8, max_keep_dim=8)
    assert e.value.code == pkg._abi.LVI_ERR_NO_DEVICE


def test_host_libraries_link_with_and_without_the_marginalizer(pkg, oracle, tmp_path):
    """the oracle-linked host library builds without the marg flattening; the HIP one exports it"""
    H = pkg.host_api
    out = tmp_path / "liblvi_host_oracle.so"
    H.build_host_library(str(out), os.path.dirname(oracle.path), "lvi_oracle", extra=("-fopenmp",))
    assert not H.HostLibrary(str(out)).has_marg
    assert "lvh_marg_" not in subprocess.run(["nm", "-D", "--defined-only", str(out)], capture_output=True, text=True).stdout
    assert os.path.exists(H.HOST_HIP_LIB), "host/liblvi_host_hip.so not built: run __graft_entry__.build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", H.HOST_HIP_LIB], capture_output=True, text=True).stdout
    for name in ("lvh_marg_create", "lvh_marg_destroy", "lvh_marg_handle", "lvh_marg_set_window", "lvh_marg_set_features", "lvh_marg_set_imu", "lvh_marg_run",
                 "lvh_marg_last_error"):
        assert re.search(r"\b%s\b" % name, syms), name
    assert H.HostLibrary(H.HOST_HIP_LIB).has_marg and H.COMPONENTS["marg"].sources == ("lvi_marg_capi.cpp",)
    assert "lvi_marg_capi.cpp" in H.component_sources()


def test_load_estimator_yaml(pkg, tmp_path):
    p = tmp_path / "params_camera.yaml"
    p.write_text("%YAML:1.0\n---\nimage_width: 640\nimage_height: 480\nestimate_td: 1\ntd: 0.002\nrolling_shutter: 1\nrolling_shutter_tr: 0.033\n")
    c = pkg.config.load_estimator_yaml(str(p))
    assert c == dict(estimate_td=True, td=0.002, rolling_shutter_tr=0.033, image_height=480.0, tr_over_row=0.033 / 480.0, half_row=240.0)
    p.write_text("%YAML:1.0\n---\nimage_height: 512\nestimate_td: 0\ntd: 0.0\nrolling_shutter: 0\nrolling_shutter_tr: 0.033\n")
    c = pkg.config.load_estimator_yaml(str(p))                  # parameters.cpp:127-135: TR = 0 without a rolling shutter
    assert c["estimate_td"] is False and c["rolling_shutter_tr"] == 0.0 and c["tr_over_row"] == 0.0 and c["half_row"] == 256.0


# ---- the reference itself ------------------------------------------------------------------------------
def _factor_cases():
    """(pose_i, pose_j, ex, inv_dep, td, observation): every observation pair of a seeded window"""
    win, feats = R.make_window(31, 4, frames_seen=[11, 4, 2, 6])
    out = []
    for f in feats:
        for j in range(1, len(f["obs"])):
            out.append((win["pose"][0], win["pose"][j], win["ex"], f["inv_dep"], win["td"], R._rec(0, j, 0, f["obs"][0], f["obs"][j])))
    return out


def _plus(p, d):
    """the reference's local parameterisation: p + dp, q * deltaQ(dtheta)"""
    q = np.array(p, np.float64)
    q[:3] += d[:3]
    dq = np.r_[d[3:] / 2, 1.0]
    q[3:] = R.quat_mul(p[3:], dq / np.linalg.norm(dq))
    return q


def jacobian_gap(use_td):
    worst = 0.0
    for pi, pj, ex, inv, td, rec in _factor_cases():
        args = [pi, pj, ex, inv, td]
        _, J = R.projection_eval(*args, use_td, rec, R.F64, tr_over_row=2e-5)
        for c in range(20 if use_td else 19):
            def ev(s):
                a = list(args)
                if c < 18:
                    d = np.zeros(6)
                    d[c % 6] = s * H_CD
                    a[c // 6] = _plus(a[c // 6], d)
                else:
                    a[c - 15] = a[c - 15] + s * H_CD
                return R.projection_eval(*a, use_td, rec, R.F64, tr_over_row=2e-5)[0]
            worst = max(worst, float(np.abs((ev(1) - ev(-1)) / (2 * H_CD) - J[:, c]).max()))
    return worst


@pytest.mark.parametrize("use_td", [1, 0])
def test_reference_jacobians_against_central_differences(use_td):
    gap = jacobian_gap(use_td)
    print(f"[marg ref] use_td {use_td}: analytic vs central differences (h = {H_CD}): {gap:.3e}, bound {JAC_GAP_BOUND:.3e}")
    assert gap <= JAC_GAP_BOUND


def test_reference_arithmetics_agree_on_the_factors():
    worst = 0.0
    for pi, pj, ex, inv, td, rec in _factor_cases()[:6]:
        for use_td in (1, 0):
            (r, J), (rm, Jm) = (R.projection_eval(pi, pj, ex, inv, td, use_td, rec, X, tr_over_row=2e-5) for X in (R.F64, R.MP))
            worst = max(worst, R.gap(r, rm), R.gap(J, Jm))
    print(f"[marg ref] float64 vs mpmath on the projection factors: {worst:.3e}")
    assert worst <= HEADER_TOL


def test_loss_correction_is_the_gradient_and_gauss_newton_of_rho():
    """with rho'' <= 0 the corrected factor has J'r = rho' J'r and J'J = rho' J'J (ceres' Corrector)"""
    rs = np.random.RandomState(3)
    for kind in (R.LOSS_CAUCHY, R.LOSS_HUBER):
        for scale in (0.1, 3.0):
            r, J = rs.normal(0, scale, 2), rs.normal(0, 1, (2, 20))
            rho = R.loss_rho(kind, 1.0, float(r @ r), R.F64)
            rc, Jc = R.loss_correct(r, J, rho, R.F64)
            assert rho[2] <= 0 and np.abs(Jc.T @ rc - rho[1] * J.T @ r).max() < 1e-13 and np.abs(Jc.T @ Jc - rho[1] * J.T @ J).max() < 1e-12
    # the second branch, with hand-given rho: J'r = rho' J'r still, and J'J = rho' J'J + 2 rho'' J'r r'J
    r, J, rho = rs.normal(0, 1, 2), rs.normal(0, 1, (2, 20)), [0.0, 0.7, 0.05]
    rc, Jc = R.loss_correct(r, J, rho, R.F64)
    assert np.abs(Jc.T @ rc - rho[1] * J.T @ r).max() < 1e-13
    assert np.abs(Jc.T @ Jc - (rho[1] * J.T @ J + 2 * rho[2] * np.outer(J.T @ r, J.T @ r))).max() < 1e-12


def test_psd_factor_reproduces_its_input():
    rs = np.random.RandomState(4)
    B = R.MP.arr(rs.normal(0, 1, (4, 9)))                                # the products in mpmath: exactly rank 4
    H, g = B.T @ B, B.T @ R.MP.arr(rs.normal(0, 1, 4))
    J, r = R.psd_factor(H, g, R.MP)
    assert R.gap(J.T @ J, H) < 1e-40 and R.gap(J.T @ r, g) < 1e-40 and all(x == 0 for x in J[4:].ravel())


# ---- the GPU tier's scenes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in R.GPU_SCENES if n not in R.SYSTEM_ONLY])
def test_gpu_scene_conditions(name):
    """Asserted here so the GPU tier cannot hide behind them: a scene used for a rank comparison has no exact (mpmath)
    eigenvalue of Amm or of the Schur complement inside [eps / 100, 100 eps], and dim x 2.2e-16 x ||A||_2 < eps / 10, so
    the threshold decisions are not rounding noise.  The other scenes are compared on H and g only."""
    f, m = R.scene_reference(name)
    clear, quiet, noise = R.scene_conditions(m)
    print(f"[marg ref] {name}: m {m['m']} n {m['n']} rank (float64, mpmath) ({f['rank']}, {m['rank']}); no eigenvalue near eps: {clear}; "
          f"dim u ||A|| = {noise:.3e} (eps / 10 = {R.EPS / 10:.1e}); G_A {R.gap(f['A'], m['A']):.3e} G_H {R.gap(f['H'], m['H']):.3e} G_g {R.gap(f['g'], m['g']):.3e}")
    if R.gpu_scene(name)["rank"]:
        assert clear and quiet and f["rank"] == m["rank"]
    else:
        assert not (clear and quiet), "the scene qualifies for a rank comparison: mark it"


def test_gpu_scene_shapes():
    shapes = {n: (R.scene_reference(n)[0]["m"], R.scene_reference(n)[0]["n"]) for n in R.GPU_SCENES}
    assert shapes["one_factor"] == (7, 13) and shapes["three_td"] == (9, 25) and shapes["three_plain"] == (9, 24)
    assert [shapes[k] for k in ("eig_3_6", "eig_7_12", "eig_4_5", "eig_1_1", "eig_2_3")] == [(3, 6), (7, 12), (4, 5), (1, 1), (2, 3)]
    # one size at and two past the eigen-solver's width: 1024 threads over (dim' / 2) x dim entries of a round
    assert [shapes[k] for k in ("eig_44_45", "eig_45_46")] == [(44, 45), (45, 46)] and 22 * 44 <= 1024 < 23 * 45
    count = {n: sum(1 for o in R.gpu_scene(n)["ops"] if o[0] == "proj") for n in R.GPU_SCENES}
    assert count["one_factor"] == 1 and count["share_plus_1"] == R.SHARE + 1 and count["two_partials_plus_1"] == 2 * R.SHARE + 1
    # the outlier of the three-feature scenes is one the loss changes: its rho' is far below 1
    sc = R.gpu_scene("three_td")
    M = R.play(dict(ops=[o for o in sc["ops"] if o[0] == "block"]), R.Marg(R.F64, loss=R.LOSS_NONE, **sc["params"]))
    s = []
    for o in sc["ops"]:
        if o[0] == "proj":
            M.factors = []
            M.add_projection(o[1])
            s.append(float(M.factors[0][1] @ M.factors[0][1]))
    assert s[2] > 100 and max(s[:2] + s[3:]) < 25 and R.loss_rho(R.LOSS_CAUCHY, 1.0, s[2], R.F64)[1] < 0.01
    assert len({o[1]["pose_j"] for o in sc["ops"] if o[0] == "proj" and o[1]["feature"] == R.ID_FEATURE}) == 3     # one feature seen from every frame
    # the untouched kept block of eig_3_6 has an exactly zero row and column already in the reference
    f, _ = R.scene_reference("eig_3_6")
    assert not f["A"][5:9].any() and not f["A"][:, 5:9].any() and not f["H"][2:6].any()


def test_chain_reference():
    """the chain of the GPU tier: its shapes, that its second step is the MARGIN_SECOND_NEW branch that runs, that the dx
    path meets a sign-flipped quaternion, and that the float64 and mpmath chains agree"""
    steps, ref = R.chain_steps(), R.chain_reference()
    assert [s[0] for s in steps] == [R.MARGIN_OLD, R.MARGIN_SECOND_NEW, R.MARGIN_OLD]
    assert (ref[0][0]["m"], ref[0][0]["n"]) == (15 + 6, 76) and (ref[1][0]["m"], ref[1][0]["n"]) == (6, 70) and ref[2][0]["n"] == 64
    assert R.ID_POSE + R.WINDOW_SIZE - 1 in ref[0][0]["ids"] and R.ID_POSE + R.WINDOW_SIZE - 1 not in ref[1][0]["ids"]
    prior, win = ref[1][0], steps[2][1]
    flipped = [b for b, x0 in zip(prior["ids"], prior["x0"]) if len(x0) == 7 and float(np.dot(x0[3:], win["pose"][b][3:] if b < 16 else win["ex"][3:])) < 0]
    assert R.ID_POSE + 3 in flipped and R.ID_EX in flipped
    for k, (f, m) in enumerate(ref):
        print(f"[marg ref] chain step {k}: m {f['m']} n {f['n']} rank ({f['rank']}, {m['rank']}); G_H {R.gap(f['H'], m['H']):.3e} G_g {R.gap(f['g'], m['g']):.3e} "
              f"||A|| {R.norm2(f['A']):.3e}; conditions {R.scene_conditions(m)[:2]}")
        assert f["ids"] == m["ids"] and R.gap(f["H"], m["H"]) < 1e-6 * R.norm2(f["A"])


# ---- csrc/lvi_marg_math.hpp alone, under the host sanitizers ------------------------------------------------
DRIVER = r"""
// stand-alone driver of csrc/lvi_marg_math.hpp and of the host helpers of csrc/lvi_winsys.hpp: the factor pieces the kernels
// call and the record checks and staging both handles call, run on the host
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <map>
#include "lvi_marg_math.hpp"
#include "lvi_winsys.hpp"
using namespace lvi_marg_math;
using namespace lvi_winsys;

static void put(const double* v, int n) { for (int i = 0; i < n; i++) std::printf(" %a", v[i]); }

// csrc/lvi_winsys.hpp's host helpers: one valid record and one of each refused kind -> 0, or the number of the case that went wrong
static int check_records()
{
    // ids 0, 1: poses, 2: extrinsic, 3: feature, 4: td, 5: an eliminated feature, 6: a speed-bias; block index = id + 10
    const std::map<int, BlockRef> table = {{0, {10, 7, false}}, {1, {11, 7, false}}, {2, {12, 7, false}}, {3, {13, 1, false}}, {4, {14, 1, false}},
                                           {5, {15, 1, true}}, {6, {16, 9, false}}};
    const auto look = [&](int id) { const auto it = table.find(id); return it == table.end() ? BlockRef{-1, 0, false} : it->second; };
    const auto find = [&](int id) { return look(id).index; };
    lvi_marg_projection ok;
    std::memset(&ok, 0, sizeof(ok));
    ok.pose_i = 0; ok.pose_j = 1; ok.ex = 2; ok.feature = 3; ok.td = 4;
    double obs[14];                                          // pts_i .. row_j are 14 doubles in a row
    for (int k = 0; k < 14; k++) obs[k] = 0.25 * k;
    std::memcpy(reinterpret_cast<char*>(&ok) + offsetof(lvi_marg_projection, pts_i), obs, sizeof(obs));
    const char* why = nullptr;
    const auto refused = [&](const lvi_marg_projection& p, bool rule, const char* msg) {
        why = nullptr;
        return check_projection(p, look, rule, &why) == LVI_ERR_INVALID_ARG && why && !std::strcmp(why, msg);
    };
    lvi_marg_projection p = ok;
    if (check_projection(p, look, true, &why) != LVI_OK) return 1;
    p.td = -1;
    if (check_projection(p, look, true, &why) != LVI_OK) return 2;
    p = ok; p.ex = 9;
    if (!refused(p, true, "a projection factor names an id that was not declared")) return 3;
    p = ok; p.pose_j = 6;
    if (!refused(p, true, "a projection factor's blocks must have sizes 7, 7, 7, 1, 1")) return 4;
    p = ok; p.td = 5;
    if (!refused(p, true, "an eliminated block outside the feature slot")) return 5;
    if (check_projection(p, look, false, &why) != LVI_OK) return 6;         // the marginaliser has no such rule
    p = ok; p.feature = 5;
    if (check_projection(p, look, true, &why) != LVI_OK) return 7;
    p = ok; p.pose_j = 0;
    if (!refused(p, true, "a projection factor names one block twice")) return 8;
    p = ok; p.row_j = INFINITY;
    if (!refused(p, true, "a projection record is not finite")) return 9;
    int col[17];
    for (int k = 0; k < 17; k++) col[k] = k == 12 ? -1 : 100 * k;           // the extrinsic is constant
    ProjDev q;
    stage_projection(ok, find, col, q);
    const int blk[5] = {10, 11, 12, 13, 14}, cols[5] = {1000, 1100, -1, 1300, 1400};
    if (std::memcmp(q.blk, blk, sizeof(blk)) || std::memcmp(q.col, cols, sizeof(cols)) || !q.use_td || std::memcmp(q.o.pts_i, ok.pts_i, 14 * sizeof(double))) return 10;
    p = ok; p.td = -1;
    stage_projection(p, find, col, q);
    if (q.use_td || q.blk[4] != 0 || q.col[4] != -1 || q.blk[3] != 13) return 11;
    const int ids[2] = {1, 6}, sizes[2] = {7, 9}, idx0[2] = {9, 0};
    PriorBlk pb[2];
    stage_prior_blocks(2, ids, sizes, idx0, find, col, pb);
    if (pb[0].size != 7 || pb[0].idx0 != 9 || pb[0].blk != 11 || pb[0].newcol != 1100 || pb[1].size != 9 || pb[1].idx0 != 0 || pb[1].blk != 16 || pb[1].newcol != 1600) return 12;
    const double v[3] = {1., NAN, 2.};
    return finite_all(v, 1) && !finite_all(v, 3) && finite_all(v + 2, 1) ? 0 : 13;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "check")) return check_records();
    if (argc < 3) return 1;
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    if (!std::strcmp(argv[1], "proj")) {
        // records: int32 use_td, int32 loss, then pose_i [7], pose_j [7], ex [7], inv_dep, td, tr_over_row, the 14 doubles of ProjObs
        int32_t hd[2];
        while (std::fread(hd, 4, 2, f) == 2) {
            double v[24 + 14];
            if (std::fread(v, 8, 38, f) != 38) return 3;
            ProjObs o;
            std::memcpy(&o, v + 24, sizeof(o));
            const ProjConst c{460.0 / 1.5, v[23], 240.0};
            double r[2], J[2 * PROJ_COLS];
            projection_eval(v, v + 7, v + 14, v[21], v[22], hd[0], o, c, r, J);
            if (hd[1] != LOSS_NONE) {
                double rho[3];
                loss_rho(hd[1], 1.0, r[0] * r[0] + r[1] * r[1], rho);
                loss_correct(2, PROJ_COLS, PROJ_COLS, rho, r, J);
            }
            put(r, 2); put(J, 2 * PROJ_COLS);
            std::printf("\n");
        }
    } else if (!std::strcmp(argv[1], "loss")) {
        // records: rho [3], r [2], J [2][20]: the correction with hand-given rho
        double v[3 + 2 + 40];
        while (std::fread(v, 8, 45, f) == 45) {
            loss_correct(2, PROJ_COLS, PROJ_COLS, v, v + 3, v + 5);
            put(v + 3, 42);
            std::printf("\n");
        }
    } else if (!std::strcmp(argv[1], "dx")) {
        // records: int32 size, x [16], x0 [16]
        int32_t size;
        while (std::fread(&size, 4, 1, f) == 1) {
            double v[32], dx[16];
            if (std::fread(v, 8, 32, f) != 32) return 3;
            prior_dx(size, v, v + 16, dx);
            put(dx, local_size(size));
            std::printf("\n");
        }
    } else if (!std::strcmp(argv[1], "rot")) {
        // records: app, aqq, apq -> c, s and the rotated off-diagonal entry
        double v[3];
        while (std::fread(v, 8, 3, f) == 3) {
            double c, s;
            jacobi_cs(v[0], v[1], v[2], &c, &s);
            const double off = c * s * (v[0] - v[1]) + (c * c - s * s) * v[2];
            const double o[3] = {c, s, off};
            put(o, 3);
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
    d = tmp_path_factory.mktemp("marg_header")
    return {"plain": _build_driver(pkg, d / "plain", []),
            "san": _build_driver(pkg, d / "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])}


def _run(exe, mode, path):
    r = subprocess.run([exe, mode, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return [np.array([float.fromhex(x) for x in l.split()]) for l in r.stdout.split("\n") if l]


def _obs14(rec):
    return np.r_[rec["pts_i"], rec["pts_j"], rec["velocity_i"], rec["velocity_j"], rec["td_i"], rec["td_j"], rec["row_i"], rec["row_j"]].astype(np.float64)


@pytest.mark.parametrize("which", ["plain", "san"])
def test_math_header_projection_factors_equal_the_reference(drivers, tmp_path, which):
    blob, want = b"", []
    for pi, pj, ex, inv, td, rec in _factor_cases():
        for use_td in (1, 0):
            for loss in (R.LOSS_NONE, R.LOSS_CAUCHY, R.LOSS_HUBER):
                blob += struct.pack("<ii", use_td, loss) + np.r_[pi, pj, ex, inv, td, 2e-5].astype(np.float64).tobytes() + _obs14(rec).tobytes()
                r, J = R.projection_eval(pi, pj, ex, inv, td, use_td, rec, R.F64, tr_over_row=2e-5)
                if loss != R.LOSS_NONE:
                    r, J = R.loss_correct(r, J, R.loss_rho(loss, 1.0, float(r @ r), R.F64), R.F64)
                want.append(np.r_[r, J.ravel()])
    (tmp_path / "p.bin").write_bytes(blob)
    got = _run(drivers[which], "proj", tmp_path / "p.bin")
    assert len(got) == len(want) >= 100
    worst = max(np.abs(g - w).max() for g, w in zip(got, want))
    print(f"[marg header] {which}: projection factors and loss vs reference {worst:.3e} (tolerance {HEADER_TOL:.3e})")
    assert worst <= HEADER_TOL
    assert all(g[2 + 19] == 0 and g[2 + 39] == 0 for g in got[3:6])          # ProjectionFactor: no td column


@pytest.mark.parametrize("which", ["plain", "san"])
def test_math_header_loss_branches_prior_dx_and_rotation(drivers, tmp_path, which):
    rs = np.random.RandomState(7)
    blob, want = b"", []
    for rho in ([0.0, 0.7, -0.05], [0.0, 0.7, 0.05], [0.0, 1.3, 0.2], [0.0, 1.0, 0.0]):       # first branch, second branch twice, the identity
        r, J = rs.normal(0, 1, 2), rs.normal(0, 1, (2, 20))
        blob += np.r_[rho, r, J.ravel()].tobytes()
        rc, Jc = R.loss_correct(r, J, rho, R.F64)
        want.append(np.r_[rc, Jc[0], Jc[1]])
    (tmp_path / "l.bin").write_bytes(blob)
    got = _run(drivers[which], "loss", tmp_path / "l.bin")
    # the driver prints r then J row-major, as the reference rows are laid out here
    worst = max(np.abs(g - w).max() for g, w in zip(got, want))
    print(f"[marg header] {which}: both loss-correction branches vs reference {worst:.3e}")
    assert len(got) == 4 and worst <= 1e-14
    blob, want, signs = b"", [], []
    for size, flip in ((7, 1), (7, -1), (7, 1), (7, -1), (9, 1), (1, 1), (16, 1)):
        x0, x = rs.normal(0, 1, 16), rs.normal(0, 1, 16)
        if size == 7:
            x0[3:7] = R.rand_quat(rs, 0.8)
            x[3:7] = flip * R.quat_mul(x0[3:7], R.rand_quat(rs, 0.2))
            signs.append(float(np.dot(x[3:7], x0[3:7])))
        blob += struct.pack("<i", size) + x.tobytes() + x0.tobytes()
        want.append(R.prior_dx(size, x[:size], x0[:size], R.F64))
    (tmp_path / "d.bin").write_bytes(blob)
    got = _run(drivers[which], "dx", tmp_path / "d.bin")
    worst = max(np.abs(g - w).max() for g, w in zip(got, want))
    print(f"[marg header] {which}: prior dx vs reference {worst:.3e}; q0.q of the size-7 cases {['%.2f' % s for s in signs]}")
    assert min(signs) < -0.5 and max(signs) > 0.5                        # a quaternion pair with w < 0 is among them
    assert [len(g) for g in got] == [6, 6, 6, 6, 9, 1, 16] and worst <= 1e-15
    assert np.abs(got[1][3:]).max() < 0.5                                # the sign branch keeps the small rotation small
    cases = [(2.0, 1.0, 0.5), (1.0, 1.0, 1e-3), (0.0, 0.0, 1.0), (5.0, -3.0, 1e-200), (1e-8, 1e8, 3.0), (-1.0, 2.0, -4.0)]
    (tmp_path / "r.bin").write_bytes(np.array(cases, np.float64).tobytes())
    got = _run(drivers[which], "rot", tmp_path / "r.bin")
    for g, (app, aqq, apq) in zip(got, cases):
        assert abs(g[0] ** 2 + g[1] ** 2 - 1) < 1e-15 and abs(g[2]) <= 4e-16 * max(abs(app), abs(aqq), abs(apq)) and abs(g[1]) <= g[0]


@pytest.mark.parametrize("which", ["plain", "san"])
def test_shared_host_helpers_check_and_stage_records(drivers, which):
    """csrc/lvi_winsys.hpp needs no HIP on its host side: the driver feeds its record check one valid record and one of every
    refused kind (with and without the window solve's eliminated-slot rule), and its staging a record and a prior's blocks"""
    r = subprocess.run([drivers[which], "check"], capture_output=True, text=True)
    assert r.returncode == 0, f"case {r.returncode}: " + r.stdout + r.stderr
