"""CPU tier of the batch tracker handle (include/lvi_tbatch.h): the header, the binding table and the product library's exports
agree, and the argument checks answer before the device is touched — so they answer on a machine without one."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "lvi_tbatch.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lvi_tbatch_[a-z0-9_]+)\s*\(", txt)))


def test_header_and_tbatch_binding_agree(pkg):
    assert _declared() == sorted(pkg.tbatch.TBATCH_SIGNATURES.keys())
    assert len(_declared()) == 16
    assert not set(_declared()) & set(pkg._abi.SIGNATURES), "the batch ABI must stay out of lvi_hotpath.h's table"
    txt = open(os.path.join(ROOT, "include", "lvi_tbatch.h")).read()
    assert int(re.search(r"#define LVI_TRACKER_MAX_BATCH\s+(\d+)", txt).group(1)) == pkg.tbatch.MAX_BATCH == 8
    assert int(re.search(r"#define LVI_TBDBG_REDO_MASK\s+(\d+)", txt).group(1)) == pkg.tbatch.TBDBG_REDO_MASK


def test_every_declaration_cites_the_call_it_batches():
    """each prototype of the header is preceded by a comment that names its lvi_tracker_* counterpart"""
    txt = open(os.path.join(ROOT, "include", "lvi_tbatch.h")).read()
    for name in _declared():
        if name == "lvi_tbatch_abi_version":
            continue
        head = txt[:re.search(r"\b" + name + r"\s*\(", txt).start()]
        last_comment = head[head.rindex("/*"):]
        assert "lvi_tracker_" in last_comment, name


def test_product_library_exports_the_batch_interface(pkg):
    lib = pkg.load_hip()
    pkg.tbatch.bind(lib)                       # AttributeError = a missing export
    assert lib.dll.lvi_tbatch_abi_version() == 1
    assert lib.dll.lvi_abi_version() == 6      # lvi_hotpath.h's version does not move


def test_slot_count_is_checked_before_the_device(pkg):
    A = pkg._abi
    lib = pkg.load_hip()
    pkg.tbatch.bind(lib)
    p = pkg.default_tracker_params(lib)
    for slots in (0, 9, -1):
        h = C.c_void_p()
        assert lib.dll.lvi_tbatch_create(C.byref(p), slots, 0, C.byref(h)) == A.LVI_ERR_INVALID_ARG, slots
        assert not h
    h = C.c_void_p()
    assert lib.dll.lvi_tbatch_create(None, 2, 0, C.byref(h)) == A.LVI_ERR_INVALID_ARG
    assert lib.dll.lvi_tbatch_create(C.byref(p), 2, 0, None) == A.LVI_ERR_INVALID_ARG
    bad = pkg.default_tracker_params(lib, lk_win=20)
    assert lib.dll.lvi_tbatch_create(C.byref(bad), 2, 0, C.byref(h)) == A.LVI_ERR_INVALID_ARG
    # null handles
    assert lib.dll.lvi_tbatch_run_lk(None) == A.LVI_ERR_INVALID_ARG
    assert lib.dll.lvi_tbatch_push_images(None, None, 8, 8, 8) == A.LVI_ERR_INVALID_ARG
    lib.dll.lvi_tbatch_destroy(None)


def test_tracker_batch_fails_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.LviError) as e:
        pkg.TrackerBatch(pkg.load_hip(), 8)
    assert e.value.code == pkg._abi.LVI_ERR_NO_DEVICE


def test_host_libraries_link_with_and_without_the_rig(pkg, oracle, tmp_path):
    """the oracle-linked host library builds without the rig's flattening; the HIP one exports it"""
    import subprocess
    H = pkg.host_api
    out = tmp_path / "liblvi_host_oracle.so"
    H.build_host_library(str(out), os.path.dirname(oracle.path), "lvi_oracle", extra=("-fopenmp",))
    assert not H.HostLibrary(str(out)).has_rig
    assert "lvh_rig_" not in subprocess.run(["nm", "-D", "--defined-only", str(out)], capture_output=True, text=True).stdout
    assert os.path.exists(H.HOST_HIP_LIB), "host/liblvi_host_hip.so not built: run __graft_entry__.build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", H.HOST_HIP_LIB], capture_output=True, text=True).stdout
    for name in ("lvh_rig_create", "lvh_rig_destroy", "lvh_rig_read_images", "lvh_rig_update_ids", "lvh_rig_reset_ids", "lvh_rig_camera",
                 "lvh_rig_use_device_fundamental", "lvh_rig_last_error"):
        assert re.search(r"\b%s\b" % name, syms), name
    assert H.HostLibrary(H.HOST_HIP_LIB).has_rig


def test_rig_fails_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = pkg.load_hip()
    with pytest.raises(pkg.LviError):
        pkg.host_api.TrackerRig(pkg.load_host(), pkg.default_tracker_params(lib), 3, 240, 320)
