"""CPU tier of the host mirror's component registry (host_api.COMPONENTS): every component links and loads
with exactly what its `needs` name, the signature tables are what the libraries export, the dependency lists are rules
that staleness acts on, and the wrappers of a host library built against the CPU oracle share one lifetime."""
import ctypes
import gc
import importlib
import os
import subprocess

import pytest

import test_host_nodes as TN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lvh_exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(s for s in (line.split()[-1] for line in out.splitlines() if line.strip()) if s.startswith("lvh_"))


def _oracle_build(pkg, oracle, out):
    return pkg.host_api.build_host_library(str(out), os.path.dirname(oracle.path), "lvi_oracle", extra=("-fopenmp",))


@pytest.fixture(scope="module")
def oracle_host(pkg, oracle, tmp_path_factory):
    return _oracle_build(pkg, oracle, tmp_path_factory.mktemp("hostlib") / "liblvi_host_oracle.so")


@pytest.fixture(scope="module")
def build_py(pkg):
    return importlib.import_module(pkg.__name__ + ".build")


def _closure(H, name):
    done, todo = set(), [name]
    while todo:
        n = todo.pop()
        if n not in done:
            done.add(n)
            todo += H.COMPONENTS[n].needs
    return done


def test_the_table_is_ordered_and_names_existing_files(pkg):
    H = pkg.host_api
    assert list(H.COMPONENTS) == ["depth", "fmat", "gmap", "loop", "kf", "bow", "pnp", "pgo", "tbatch", "marg", "win", "fman"]
    for name, c in H.COMPONENTS.items():
        assert c.sources and all(os.path.exists(os.path.join(H.HOST_DIR, f)) for f in c.sources), name
        assert all(n in H.COMPONENTS for n in c.needs), name
        assert c.probe in c.signatures and c.last_error in c.signatures, name
    assert {n: c.flag for n, c in H.COMPONENTS.items() if c.flag != "has_" + n} == {"tbatch": "has_rig"}
    assert H.COMPONENTS["tbatch"].probe == "lvh_rig_create" and H.COMPONENTS["fmat"].probe == "lvh_trk_use_device_fundamental"
    every = H.component_sources()
    assert every == tuple(f for c in H.COMPONENTS.values() for f in c.sources) and len(set(every)) == len(every)
    assert H.component_sources(["fman"]) == ("lvi_marg_capi.cpp", "lvi_win_capi.cpp", "lvi_fman_capi.cpp")
    assert H.component_sources(["pnp", "bow", "pnp"]) == ("lvi_bow_capi.cpp", "lvi_pnp_capi.cpp")
    assert H.component_sources([]) == ()


@pytest.mark.parametrize("name", ["depth", "fmat", "gmap", "loop", "kf", "bow", "pnp", "pgo", "tbatch", "marg", "win", "fman"])
def test_a_component_links_and_loads_with_what_it_needs(pkg, build_py, tmp_path, name):
    """RTLD_NOW makes an unresolved lvh_* or C++ symbol a load error; binding makes a missing export an AttributeError"""
    H = pkg.host_api
    out = tmp_path / f"liblvi_host_{name}.so"
    H.build_host_library(str(out), build_py.CSRC, "lvi_hip", extra=("-O0",), sources=H.component_sources([name]))
    hl = H.HostLibrary(str(out))
    want = _closure(H, name)
    assert {n for n, c in H.COMPONENTS.items() if getattr(hl, c.flag)} == want
    tables = [H.CORE_SIGNATURES] + [H.COMPONENTS[n].signatures for n in want]
    assert _lvh_exports(str(out)) == sorted([s for t in tables for s in t] + list(H.INTERNAL_EXPORTS))


def test_exports_equal_the_tables(pkg, oracle_host):
    H = pkg.host_api
    assert os.path.exists(H.HOST_HIP_LIB), "host/liblvi_host_hip.so not built: run __graft_entry__.build()"
    names = list(H.CORE_SIGNATURES) + [s for c in H.COMPONENTS.values() for s in c.signatures]
    assert len(names) == len(set(names)) == 116
    assert _lvh_exports(H.HOST_HIP_LIB) == sorted(names + list(H.INTERNAL_EXPORTS))
    assert _lvh_exports(oracle_host) == sorted(list(H.CORE_SIGNATURES) + list(H.INTERNAL_EXPORTS))
    hl = H.HostLibrary(oracle_host)
    assert not any(getattr(hl, c.flag) for c in H.COMPONENTS.values())


def test_every_table_entry_is_a_restype_argtypes_pair(pkg):
    H = pkg.host_api
    simple = type(ctypes.c_int)                              # the metaclasses of ctypes' scalar and pointer types
    pointer = type(ctypes.POINTER(ctypes.c_int))
    for table in [H.CORE_SIGNATURES] + [c.signatures for c in H.COMPONENTS.values()]:
        for name, entry in table.items():
            assert isinstance(entry, tuple) and len(entry) == 2, name
            res, args = entry
            assert res is None or isinstance(res, simple), name
            assert isinstance(args, list), name
            for a in args:
                assert isinstance(a, (simple, pointer, type(H.FUNDAMENTAL_FN))), (name, a)


def test_dependency_lists_are_rules(pkg, build_py):
    H = pkg.host_api
    deps = H.host_dependencies(H.component_sources())
    assert os.path.join(H.HOST_DIR, "lvi_gps_gate.hpp") in deps and os.path.join(ROOT, "include", "lvi_pgo_gps.h") in deps
    headers = sorted(os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    assert headers and set(headers) <= set(deps) and set(headers) <= set(build_py.hip_dependencies())
    for f in os.listdir(H.HOST_DIR):
        if f.endswith(".hpp") or f in ("lvi_seq_capi.cpp",) + H.component_sources():
            assert os.path.join(H.HOST_DIR, f) in deps, f
    for f in os.listdir(build_py.CSRC):
        if f.endswith((".hip", ".hpp")):
            assert os.path.join(build_py.CSRC, f) in build_py.hip_dependencies(), f
    assert all(os.path.exists(d) for d in deps + build_py.hip_dependencies())
    # no host file includes anything of the project's from outside host/ and include/
    for f in os.listdir(H.HOST_DIR):
        if f.endswith((".hpp", ".cpp")):
            for line in open(os.path.join(H.HOST_DIR, f)):
                if line.startswith('#include "'):
                    inc = os.path.normpath(os.path.join(H.HOST_DIR, line.split('"')[1]))
                    assert os.path.dirname(inc) in (H.HOST_DIR, os.path.join(ROOT, "include")), (f, line)


def test_staleness_acts_on_the_dependencies(pkg, oracle, tmp_path):
    H = pkg.host_api
    out = str(_oracle_build(pkg, oracle, tmp_path / "liblvi_host_oracle.so"))
    t = os.path.getmtime(os.path.join(H.HOST_DIR, "lvi_gps_gate.hpp")) - 1.0
    os.utime(out, (t, t))                                    # the output, never a file of the repository
    assert os.path.getmtime(out) == t
    _oracle_build(pkg, oracle, out)
    fresh = os.path.getmtime(out)
    assert fresh > t
    _oracle_build(pkg, oracle, out)
    assert os.path.getmtime(out) == fresh


def test_one_lifetime_on_the_cpu(pkg, oracle, oracle_host):
    """close() twice, then del, raises nothing; an object dropped without close() is finalised"""
    H = pkg.host_api
    hl = H.HostLibrary(oracle_host)
    w, h = 240, 180
    tp = pkg.default_tracker_params(oracle, max_width=w, max_height=h, max_cnt=60, min_dist=12.0)

    def node():
        return H.TrackerNode(hl, tp, h, w, 10, equalize=False, cam=TN.CAM)

    def mapper():
        return H.SequentialMapper(hl, oracle, pkg.default_params(oracle, **TN.SEQ_P), incremental_map=1)

    for make, ptr in ((node, "_t"), (mapper, "_s")):
        cls = type(make())
        assert issubclass(cls, pkg._abi.Owned) and "close" not in vars(cls) and "__del__" not in vars(cls)
        real, freed = getattr(hl.dll, cls._destroy), []
        setattr(hl.dll, cls._destroy, lambda p: freed.append(p) or real(p))           # counts what reaches the C++ side
        try:
            a = make()
            assert getattr(a, ptr) and not freed
            a.close()
            assert not getattr(a, ptr) and len(freed) == 1
            a.close()
            del a
            gc.collect()
            assert len(freed) == 1
            b = make()
            held = getattr(b, ptr)
            del b
            gc.collect()
            assert freed[1:] == [held]
        finally:
            setattr(hl.dll, cls._destroy, real)
