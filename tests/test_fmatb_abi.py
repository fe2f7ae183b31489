"""CPU tier of the batched device RANSAC (include/lvi_fmatb.h): the header, the binding table and the product
library's exports agree, the ABIs beside it do not move, the argument checks answer before the device is touched, and
rejectWithF's two halves (FeatureTrackerState::prepareRejectWithF / applyRejectWithF) leave what rejectWithF leaves."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", _header("lvi_fmatb.h"), flags=re.S)
    return sorted(set(re.findall(r"\b(lvi_fmatb_[a-z0-9_]+)\s*\(", txt)))


def test_header_and_fmatb_binding_agree(pkg):
    assert _declared() == sorted(pkg.fmatb.FMATB_SIGNATURES.keys())
    assert len(_declared()) == 7
    for table in (pkg.fmat.FMAT_SIGNATURES, pkg.tbatch.TBATCH_SIGNATURES, pkg._abi.SIGNATURES):
        assert not set(_declared()) & set(table), "the batched RANSAC's ABI must stay out of the other tables"
    assert int(re.search(r"#define LVI_FMATB_ABI_VERSION\s+(\d+)", _header("lvi_fmatb.h")).group(1)) == 1
    # the slot limit is the tracker batch's, not a second constant
    assert not re.search(r"#define\s+LVI_FMATB_MAX", _header("lvi_fmatb.h"))
    assert "LVI_TRACKER_MAX_BATCH" in _header("lvi_fmatb.h") and pkg.fmatb.MAX_BATCH is pkg.tbatch.MAX_BATCH


def test_the_other_headers_do_not_know_the_batched_ransac():
    for name in ("lvi_fmat.h", "lvi_tbatch.h", "lvi_hotpath.h"):
        assert "lvi_fmatb" not in _header(name).lower(), name


def test_every_declaration_cites_the_reference_call():
    """each prototype of the header is preceded by a comment that names feature_tracker.cpp:229, as lvi_fmat.h's head does"""
    txt = _header("lvi_fmatb.h")
    for name in _declared():
        if name == "lvi_fmatb_abi_version":
            continue
        head = txt[:re.search(r"\b" + name + r"\s*\(", txt).start()]
        assert "feature_tracker.cpp:229" in head[head.rindex("/*"):], name


def test_product_library_exports_the_batched_ransac_and_the_oracle_does_not(pkg, oracle):
    lib = pkg.load_hip()
    pkg.fmatb.bind(lib)                        # AttributeError = a missing export
    assert lib.dll.lvi_fmatb_abi_version() == 1
    pkg.fmat.bind(lib)
    assert lib.dll.lvi_fmat_abi_version() == 1
    assert lib.dll.lvi_abi_version() == 6
    syms = subprocess.run(["nm", "-D", "--defined-only", pkg.HIP_LIB_PATH], capture_output=True, text=True).stdout
    for name in _declared():
        assert re.search(r"\b%s\b" % name, syms), name
    assert "lvi_fmatb" not in subprocess.run(["nm", "-D", oracle.path], capture_output=True, text=True).stdout


def test_arguments_are_checked_before_the_device(pkg):
    A = pkg._abi
    lib = pkg.load_hip()
    pkg.fmatb.bind(lib)
    dll = lib.dll
    for slots, P, I in ((0, 64, 100), (9, 64, 100), (-1, 64, 100), (2, 6, 100), (2, 3073, 100), (2, 64, 0), (2, 64, 4097)):
        h = C.c_void_p()
        assert dll.lvi_fmatb_create(0, slots, P, I, C.byref(h)) == A.LVI_ERR_INVALID_ARG, (slots, P, I)
        assert not h
    assert dll.lvi_fmatb_create(0, 2, 64, 100, None) == A.LVI_ERR_INVALID_ARG
    # null handles
    assert dll.lvi_fmatb_find(None, None, None, None, None, 0.99, None, None) == A.LVI_ERR_INVALID_ARG
    assert dll.lvi_fmatb_set_check_subset(None, 1) == A.LVI_ERR_INVALID_ARG
    assert dll.lvi_fmatb_trace(None, 0, None, None, None, None, 0, None) == A.LVI_ERR_INVALID_ARG
    assert dll.lvi_fmatb_counters(None, None, None, None, None) == A.LVI_ERR_INVALID_ARG
    dll.lvi_fmatb_destroy(None)


def test_batch_fails_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.LviError) as e:
        pkg.FundamentalRansacBatch(pkg.load_hip(), 8)
    assert e.value.code == pkg._abi.LVI_ERR_NO_DEVICE


def test_host_libraries_link_with_and_without_the_batched_hook(pkg, oracle, tmp_path):
    """the HIP host library exports the rig's batched hook; a host library built against the oracle has no rig at all"""
    H = pkg.host_api
    assert os.path.exists(H.HOST_HIP_LIB), "host/liblvi_host_hip.so not built: run __graft_entry__.build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", H.HOST_HIP_LIB], capture_output=True, text=True).stdout
    for name in ("lvh_rig_use_batched_fundamental", "lvh_rig_use_device_fundamental", "lvh_rig_fundamental_stats"):
        assert re.search(r"\b%s\b" % name, syms), name
    out = tmp_path / "liblvi_host_oracle.so"
    H.build_host_library(str(out), os.path.dirname(oracle.path), "lvi_oracle", extra=("-fopenmp",))
    assert "lvh_rig_" not in subprocess.run(["nm", "-D", "--defined-only", str(out)], capture_output=True, text=True).stdout


# FeatureTrackerState alone (no handle, no library): rejectWithF() against prepareRejectWithF + the hook + applyRejectWithF on
# two states filled alike, with a hook that rejects every third point
_SPLIT_MAIN = r"""
#include <cstdio>
#include <cstring>
#include "lvi_host.hpp"
using namespace lvi_host;

static int g_calls = 0;
static std::vector<Point2f> g_a[2], g_b[2];
static double g_thr[2];

static void hook_for(int which, const std::vector<Point2f>& a, const std::vector<Point2f>& b, double thr, std::vector<uint8_t>& status)
{
    g_calls++;
    g_a[which] = a; g_b[which] = b; g_thr[which] = thr;
    status.assign(a.size(), 1);
    for (size_t i = 0; i < status.size(); i += 3) status[i] = 0;
}

static FeatureTrackerState make(int n, bool with_cam)
{
    FeatureTrackerState s(480, 752, 150, 30);
    if (with_cam) {
        lvi_mei_params cam{};
        cam.xi = 1.9926618269451453; cam.k1 = -0.0399258932468764; cam.k2 = 0.15160828121223818; cam.p1 = 0.00017756967825777937;
        cam.p2 = -0.0011531239076798612; cam.gamma1 = 669.8940458885896; cam.gamma2 = 669.1450614220616; cam.u0 = 377.9; cam.v0 = 279.6;
        s.setCamera(cam);
    }
    s.F_THRESHOLD = 0.75;
    for (int i = 0; i < n; i++) {
        s.prev_pts.push_back(Point2f{30.f + 17.f * i, 40.f + 9.5f * i});
        s.cur_pts.push_back(Point2f{31.f + 17.f * i, 41.25f + 9.5f * i});
        s.forw_pts.push_back(Point2f{32.5f + 17.f * i, 42.f + 9.5f * i});
        s.ids.push_back(100 + i); s.track_cnt.push_back(2 + i % 5);
    }
    return s;
}

template <class T> static bool same(const std::vector<T>& x, const std::vector<T>& y)
{
    return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), sizeof(T) * x.size()) == 0);
}

// returns the number of hook calls each form made, or -1 on a difference
static int run(int n, bool with_cam, int want_skipped)
{
    FeatureTrackerState whole = make(n, with_cam), halves = make(n, with_cam);
    g_calls = 0;
    whole.findFundamentalMat = [](const std::vector<Point2f>& a, const std::vector<Point2f>& b, double thr, std::vector<uint8_t>& st) { hook_for(0, a, b, thr, st); };
    whole.rejectWithF();
    const int calls_whole = g_calls;
    g_calls = 0;
    std::vector<Point2f> ua, ub;
    if (halves.prepareRejectWithF(ua, ub)) {
        std::vector<uint8_t> st(ua.size(), 1);
        hook_for(1, ua, ub, halves.F_THRESHOLD, st);
        halves.applyRejectWithF(st);
    }
    if (g_calls != calls_whole) return -1;
    if (calls_whole && !(same(g_a[0], g_a[1]) && same(g_b[0], g_b[1]) && g_thr[0] == g_thr[1] && g_a[0].size() == (size_t)n)) return -1;
    if (!(same(whole.prev_pts, halves.prev_pts) && same(whole.cur_pts, halves.cur_pts) && same(whole.forw_pts, halves.forw_pts) && same(whole.ids, halves.ids) &&
          same(whole.track_cnt, halves.track_cnt))) return -1;
    if (whole.rejectWithF_skipped != want_skipped || halves.rejectWithF_skipped != want_skipped) return -1;
    const size_t kept = calls_whole ? (size_t)(n - (n + 2) / 3) : (size_t)n;
    if (whole.forw_pts.size() != kept || whole.rejectWithF_removed != n - (int)kept || halves.rejectWithF_removed != n - (int)kept) return -1;
    return calls_whole;
}

int main()
{
    std::printf("n7 %d\n", run(7, true, 0));            // < 8: no call, no skip
    std::printf("n8 %d\n", run(8, true, 0));
    std::printf("n40 %d\n", run(40, true, 0));
    std::printf("nocam %d\n", run(8, false, 1));        // no camera: a counted skip, no call
    // no hook at all: rejectWithF() counts the skip it always counted
    FeatureTrackerState s = make(8, true);
    s.rejectWithF();
    std::printf("nohook %d %d\n", s.rejectWithF_skipped, (int)s.forw_pts.size());
    return 0;
}
"""


def test_reject_with_f_in_two_halves_equals_reject_with_f(pkg, tmp_path):
    src = tmp_path / "split_main.cpp"
    src.write_text(_SPLIT_MAIN)
    exe = tmp_path / "split_main"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(pkg.PKG_DIR, "host"), "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:5] == ["n7 0", "n8 1", "n40 1", "nocam 0", "nohook 1 8"], r.stdout
