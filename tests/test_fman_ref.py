"""CPU tier of the feature table (include/lvi_fman.h): the ABI checks, the reference tests/fman_ref.py on
constructed scenes, csrc/lvi_fman_math.hpp compiled alone (plain and as a stand-alone program under the host sanitizers)
against mpmath with the bar of the GPU tier, and the invariants of the reference's operations on random sequences."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import fman_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "lvi_fman.h")).read()


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(lvi_fman_[a-z0-9_]+)\s*\(", txt)))


# ---- ABI -------------------------------------------------------------------------------------------
def test_header_and_fman_binding_agree(pkg):
    F = pkg.fman
    assert _declared() == sorted(F.FMAN_SIGNATURES.keys())
    assert len(_declared()) == 19
    assert not set(_declared()) & set(pkg._abi.SIGNATURES) and not set(_declared()) & set(pkg.marg.MARG_SIGNATURES) and \
        not set(_declared()) & set(pkg.win.WIN_SIGNATURES)
    txt = _header()
    for name, val in (("ABI_VERSION", 1), ("MAX_FEATURES", F.MAX_FEATURES), ("WINDOW", F.WINDOW), ("MAX_OBS", F.MAX_OBS), ("MAX_SWEEPS", F.MAX_SWEEPS),
                      ("MODE_WINDOW", F.MODE_WINDOW), ("MODE_MARG_OLD", F.MODE_MARG_OLD)):
        assert int(re.search(r"#define LVI_FMAN_%s\s+(\d+)" % name, txt).group(1)) == val, name
    assert (F.MAX_FEATURES, F.WINDOW, F.MAX_OBS) == (4096, 10, 11) and (F.WINDOW, F.MAX_OBS) == (R.WINDOW, R.MAX_OBS)
    assert (F.MODE_WINDOW, F.MODE_MARG_OLD) == (R.MODE_WINDOW, R.MODE_MARG_OLD)
    assert (F.ID_POSE, F.ID_EX, F.ID_TD, F.ID_FEATURE) == (R.ID_POSE, R.ID_EX, R.ID_TD, R.ID_FEATURE)
    # every entry point cites the lines it restates
    assert all(s in txt for s in (":45-106", ":381-414", ":129-148", ":150-168", ":170-179", ":181-192", ":194-211", ":213-268", ":285-339", ":341-357",
                                  ":359-379", "estimator.cpp:745-789", ":849-889", "feature_manager.h:60-74", ":23-26", ":28-42"))
    assert '#include "lvi_marg.h"' in txt and "typedef struct lvi_marg_projection" not in txt       # the record is included, not copied
    for other in ("lvi_hotpath.h", "lvi_marg.h", "lvi_win.h"):
        assert "lvi_fman" not in open(os.path.join(ROOT, "include", other)).read(), other
    # the host mirror's id bases are the marginaliser's
    hpp = open(os.path.join(pkg.PKG_DIR, "host", "lvi_marg_host.hpp")).read()
    assert "ID_POSE = 0, ID_SPEEDBIAS = 16, ID_EX = 32, ID_TD = 33, ID_FEATURE = 64" in hpp


def test_record_layouts(pkg):
    F = pkg.fman
    txt = _header()
    for cname, cls, size in (("lvi_fman_params", F.FmanParams, 16), ("lvi_fman_frame_info", F.FmanFrameInfo, 24), ("lvi_fman_tri_info", F.FmanTriInfo, 16),
                             ("lvi_fman_ids", F.FmanIds, 16)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in re.findall(r"\b(?:int32_t|double)\s+([^;]+);", body) for n in re.findall(r"([A-Za-z_][A-Za-z_0-9]*)(?:\[\d+\])?\s*(?:,|$)", decl)]
        assert names == [f[0] for f in cls._fields_], cname
        assert ctypes.sizeof(cls) == size, cname
    assert F.OBS_DTYPE.itemsize == 72 and F.FEATURE_DTYPE.itemsize == 824
    assert list(F.OBS_DTYPE.names) == ["point", "uv", "velocity", "depth", "cur_td"]
    assert list(F.FEATURE_DTYPE.names) == ["feature_id", "start_frame", "n_obs", "lidar_depth_flag", "solve_flag", "reserved", "estimated_depth", "obs"]
    assert F.FEATURE_DTYPE.fields["estimated_depth"][1] == 24 and F.FEATURE_DTYPE.fields["obs"][1] == 32


def test_hip_library_exports_the_fman_abi_and_the_oracle_does_not(pkg, oracle):
    dll = ctypes.CDLL(pkg.HIP_LIB_PATH)
    for name in _declared():
        assert hasattr(dll, name), f"{name} missing from liblvi_hip.so"
    lib = pkg.fman.bind(pkg.load_hip())
    assert lib.dll.lvi_fman_abi_version() == 1 and lib.dll.lvi_win_abi_version() == 1 and lib.dll.lvi_marg_abi_version() == 1 and lib.dll.lvi_abi_version() == 6
    p = pkg.fman.FmanParams()
    lib.dll.lvi_fman_params_default(ctypes.byref(p))
    assert (p.init_depth, p.min_parallax) == (R.INIT_DEPTH, R.MIN_PARALLAX) == (5.0, 10.0 / 460.0)
    syms = subprocess.run(["nm", "-D", "--defined-only", oracle.path], capture_output=True, text=True).stdout
    assert "lvi_abi_version" in syms and "lvi_fman_" not in syms


def test_feature_table_fails_loudly_without_gpu(pkg):
    """no CPU fallback: without a device the handle is refused; arguments are refused before the device is looked for"""
    import torch
    lib = pkg.load_hip()
    for bad in (0, pkg.fman.MAX_FEATURES + 1):
        with pytest.raises(pkg.LviError) as e:
            pkg.FeatureTable(lib, max_features=bad)
        assert e.value.code == pkg._abi.LVI_ERR_INVALID_ARG
    if not torch.cuda.is_available():
        with pytest.raises(pkg.LviError) as e:
            pkg.FeatureTable(lib, max_features=8)
        assert e.value.code == pkg._abi.LVI_ERR_NO_DEVICE


def test_host_libraries_link_with_and_without_the_feature_manager(pkg, oracle, tmp_path):
    """the oracle-linked host library builds without the feature manager's flattening; the HIP one exports it"""
    H = pkg.host_api
    out = tmp_path / "liblvi_host_oracle.so"
    H.build_host_library(str(out), os.path.dirname(oracle.path), os.path.splitext(os.path.basename(oracle.path))[0][3:])
    assert not H.HostLibrary(str(out)).has_fman
    assert H.COMPONENTS["fman"].sources == ("lvi_fman_capi.cpp",) and pkg.load_host().has_fman
    b = importlib.import_module(pkg.__name__ + ".build")
    assert "lvi_fman.hip" in b.SOURCES and os.path.join(ROOT, "include", "lvi_fman.h") in b.hip_dependencies()
    closure = H.component_sources(["fman"])
    assert set(H.COMPONENTS["marg"].sources + H.COMPONENTS["win"].sources + H.COMPONENTS["fman"].sources) <= set(closure)
    assert set(closure) <= set(H.component_sources())              # which is what build.build_host links


# ---- the reference on constructed scenes -------------------------------------------------------------
def test_noise_free_triangulation_returns_the_constructed_depth():
    sc = R.window_scene(12, 60, noise=0.0)
    fm = R.FeatureManager()
    R.load(fm, sc["frames"])
    worst = 0.0
    for f in fm.triangulate(sc["Ps"], sc["Rs"], sc["tic"], sc["ric"]):
        worst = max(worst, abs(f.estimated_depth - sc["depth"][f.feature_id]) / sc["depth"][f.feature_id])
    print(f"[fman ref] noise-free triangulation: worst relative error {worst:.3e}")
    assert fm.get_feature_count() >= 40 and worst <= 1e-12


@pytest.mark.parametrize("name", R.TRI_SCENES)
def test_float64_svd_against_mpmath(name):
    """G of every scene the GPU tier triangulates, and the conditions those tests rely on"""
    r = R.tri_reference(name)
    print(f"[fman ref] scene {name}: {len(r['ids'])} features to triangulate, G {r['G']:.3e}, smallest gap {min(r['gaps']):.3e}")
    assert len(r["ids"]) >= 10 and 0 < r["G"] < 1e-11
    if name == "main":
        # (sigma_3 - sigma_4) / sigma_1 >= 1e-2 for every feature: no feature is excluded
        assert len(r["ids"]) == 400 and min(r["gaps"]) >= 1e-2
        n_obs = {len(f.obs) for f in r["fm"].feature}
        assert n_obs == set(range(2, 12))
    if name == "shapes":
        seen = {(f.start_frame, len(f.obs)) for f in r["fm"].feature}
        assert {(0, 2), (0, 3), (0, 11), (7, 2), (7, 3), (8, 2), (8, 3)} <= seen
        assert all(f.start_frame != 8 for f in r["fm"].to_triangulate()) and any(f.start_frame == 8 for f in r["fm"].feature)
    if name == "sign":
        neg = [k for k, i in enumerate(r["ids"]) if i % 2 == 1]
        pos = [k for k, i in enumerate(r["ids"]) if i % 2 == 0]
        assert len(neg) == len(pos) == 20
        assert all(r["exact"][k] <= -1 and r["numpy"][k] <= -1 for k in neg) and all(r["exact"][k] >= 1 and r["numpy"][k] >= 1 for k in pos)
    if name == "slot":
        assert r["fm"].feature[R.SLOT_TARGET].feature_id == R.SLOT_TARGET and R.SLOT_TARGET in r["ids"]
    if name == "still":
        flat = [k for k in range(len(r["ids"])) if r["gaps"][k] < 1e-12]
        assert len(flat) >= 8 and len(flat) < len(r["ids"])


# ---- csrc/lvi_fman_math.hpp alone, plain and under the host sanitizers ------------------------------------------
DRIVER = r"""
// stand-alone driver of csrc/lvi_fman_math.hpp: the triangulation as the kernel calls it, run on the host
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lvi_fman_math.hpp"
using namespace lvi_fman_math;
int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    Poses W;
    if (fread(&W, sizeof(double), 144, f) != 144) return 4;
    double head[2];
    while (fread(head, sizeof(double), 2, f) == 2) {
        const int start = (int)head[0], k = (int)head[1];
        if (start < 0 || k < 1 || start + k > MAX_OBS) return 5;
        std::vector<double> obs((size_t)k * OBS_DOUBLES);
        if (fread(obs.data(), sizeof(double), obs.size(), f) != obs.size()) return 6;
        int sweeps = 0;
        const double d = triangulate_depth(W, start, k, obs.data(), &sweeps);
        printf("%a %d\n", d, sweeps);
    }
    fclose(f);
    // the other functions of the header, on fixed arguments
    const double pi[3] = {0.3, -0.2, 2.0}, pj[3] = {0.1, 0.05, 1.0};
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, P0[3] = {0.5, 0, 0}, P1[3] = {0, 0, 0.25};
    printf("%a %a\n", compensated_parallax2(pi, pj), shifted_depth(pj, 4.0, I, P0, I, P1));
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
    d = tmp_path_factory.mktemp("fman_header")
    return {"plain": _build_driver(pkg, d / "plain", []),
            "san": _build_driver(pkg, d / "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])}


def _scene_blob(r):
    sc = r["scene"]
    blob = np.r_[sc["Ps"].ravel(), sc["Rs"].ravel(), sc["tic"], sc["ric"].ravel()].astype(np.float64).tobytes()
    for f in r["fm"].to_triangulate():
        blob += np.r_[float(f.start_frame), float(len(f.obs)), np.asarray(f.obs, np.float64).ravel()].tobytes()
    return blob


@pytest.mark.parametrize("which", ["plain", "san"])
@pytest.mark.parametrize("name", R.TRI_SCENES)
def test_math_header_triangulation_against_mpmath(drivers, tmp_path, which, name):
    """the bar of the device: 10 G of that scene, never below 16 ulp; the sanitizer build must exit clean"""
    r = R.tri_reference(name)
    (tmp_path / "s.bin").write_bytes(_scene_blob(r))
    out = subprocess.run([drivers[which], str(tmp_path / "s.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l.split() for l in out.stdout.split("\n") if l]
    assert len(lines) == len(r["ids"]) + 1
    bar, worst, sweeps = R.tri_bar(r["G"]), 0.0, 0
    for k, (d, s) in enumerate(lines[:-1]):
        d, s = float.fromhex(d), int(s)
        if r["gaps"][k] < 1e-6:                                    # rank 2: two columns of rounding noise, ended by the sweep bound at the latest
            assert (np.isfinite(d) or np.isnan(d)) and 1 <= s <= 30
            continue
        sweeps = max(sweeps, s)
        assert 1 <= s < 30, (name, r["ids"][k], s)                 # the stop rule ended it, not the sweep bound
        worst = max(worst, R.rel_dev(d, r["exact"][k]))
    print(f"[fman header] {which} {name}: G {r['G']:.3e}, bar {bar:.3e}, worst deviation from mpmath {worst:.3e}, most sweeps {sweeps}")
    assert worst <= bar
    par, dep = (float.fromhex(v) for v in lines[-1])
    assert par == R.compensated_parallax2([0.3, -0.2, 2.0], [0.1, 0.05, 1.0])
    eye = [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]
    assert dep == R.shifted_depth([0.1, 0.05, 1.0], 4.0, eye, [0.5, 0, 0], eye, [0, 0, 0.25]) == 3.75


# ---- invariants of the operations on random sequences -------------------------------------------------------
def _ids(fm):
    return [f.feature_id for f in fm.feature]


def _check_invariants(fm, before, appended=False):
    """before: the ids before the operation.  A frame leaves them as a prefix and appends in ascending id order; every
    other operation leaves a subsequence."""
    ids = _ids(fm)
    assert len(set(ids)) == len(ids)
    if appended:
        assert ids[:len(before)] == before and sorted(ids[len(before):]) == ids[len(before):], "list order is not preserved"
    else:
        assert [i for i in before if i in set(ids)] == ids, "list order is not preserved"
    assert all(1 <= len(f.obs) and 0 <= f.start_frame and f.start_frame + len(f.obs) <= R.MAX_OBS for f in fm.feature)
    n = fm.get_feature_count()
    for mode in (R.MODE_WINDOW, R.MODE_MARG_OLD):
        p = fm.projections(mode)
        assert len(fm.depth_vector()) == n == len(p["inv_dep"]) == len(p["lidar_flags"])
        want = sum(len(f.obs) - 1 for f in fm.feature if R.eligible(len(f.obs), f.start_frame) and (mode == R.MODE_WINDOW or f.start_frame == 0))
        assert len(p["records"]) == want
        assert all(R.ID_FEATURE <= r["feature"] < R.ID_FEATURE + n and r["pose_i"] < r["pose_j"] <= R.ID_POSE + R.WINDOW for r in p["records"])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_operation_sequences_keep_the_invariants(seed):
    rs = np.random.RandomState(seed)
    seq = R.sequence(seed, n_frames=30, per_frame=40)
    fm, frame_count, seen = R.FeatureManager(), 0, set()
    for ids, obs in seq["frames"]:
        before = _ids(fm)
        info = fm.add_frame(frame_count, ids, obs, 0.01 * seed)
        assert info["last_track_num"] + info["added"] == len(ids)
        _check_invariants(fm, before, appended=True)
        if frame_count < R.WINDOW:
            frame_count += 1
            continue
        x = np.array(fm.depth_vector())
        x[rs.uniform(size=len(x)) < 0.1] *= -1.0
        fm.set_depth(x)
        before = _ids(fm)
        what = rs.randint(0, 3)
        if what == 0:
            I3 = np.eye(3)
            seen |= set(fm.remove_back_shift_depth(I3, [0.0, 0, 0], I3, [0.08, 0, 0]))
        elif what == 1:
            seen |= set(fm.remove_back())
        else:
            seen |= set(fm.remove_front(frame_count))
        _check_invariants(fm, before)
        fm.remove_failures()
        assert all(f.solve_flag != 2 for f in fm.feature)
        _check_invariants(fm, before)
    assert {"shifted", "erased", "dep_j", "lidar", "newest", "skipped", "cut"} <= seen, seen
