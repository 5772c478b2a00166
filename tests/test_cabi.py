"""The C-ABI library loads and exports every symbol include/owlknn.h declares (no GPU needed)."""
import ctypes
import os
import re
import sys

import pytest
import torch  # noqa: F401  before the library is loaded: torch brings its own HIP runtime, and a process that loads the
#                            system's first ends up with two, of which the second to start finds no device

from owlraytracing_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cabi_calls as cc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"TKNN_API[^;(]*?\b(tknn\w+)\s*\(", text))


def test_library_exports_every_declared_symbol():
    names = _declared("owlknn.h")
    assert names, "header parse found nothing"
    lib = _lib.load()
    for name in sorted(names):
        assert hasattr(lib, name), "libowl_mi355x.so lacks %s" % name
    assert names == set(_lib.SIGNATURES), "python binding and header disagree"


def test_neigh_record_is_24_bytes():
    text = open(os.path.join(ROOT, "include", "owlknn.h")).read()
    assert "int32_t pad_" in text and "int64_t intersections" in text
    from owlraytracing_amd.trueknn import NEIGH_BYTES
    assert NEIGH_BYTES == 24


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from owlraytracing_amd.trueknn import TrueKNN
    with pytest.raises(RuntimeError):
        TrueKNN()
    # and straight through the C-ABI: creation fails with a HIP error, it does not return a CPU engine
    import ctypes
    h = ctypes.c_void_p()
    rc = _lib.load().tknnCreate(ctypes.byref(h))
    assert rc != 0 and not h.value


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "owlraytracing_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert not re.search(r'#include\s+[<"].*oracle', src), f


def test_ctypes_structs_have_the_header_layout(tmp_path):
    """Sizes and field offsets of the ctypes mirrors against include/owlknn.h compiled by gcc as C99."""
    import subprocess
    pairs = {"tknnSolveInfo": _lib.SolveInfo, "tknnSolveOptions": _lib.SolveOptions,
             "tknnDbscanInfo": _lib.DbscanInfo, "tknnDbscanAutoInfo": _lib.DbscanAutoInfo, "tknnBuildInfo": _lib.BuildInfo,
             "tknnTreeExport": _lib.TreeExport, "tknnQueryOptions": _lib.QueryOptions, "tknnDbscanQueryOptions": _lib.DbscanQueryOptions,
             "tknnRadiusOptions": _lib.RadiusOptions, "tknnRadiusInfo": _lib.RadiusInfo, "tknnRadiusKnnOptions": _lib.RadiusKnnOptions,
             "tknnRadiusKnnInfo": _lib.RadiusKnnInfo}
    mirrors = {c for c in vars(_lib).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and getattr(c, "_fields_", None)}
    assert mirrors == set(pairs.values()), "a ctypes structure of _lib is not compared with the header"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        cname, what, value = line.split()
        cls = pairs[cname]
        if what == "size":
            assert ctypes.sizeof(cls) == int(value), cname
        else:
            assert getattr(cls, what).offset == int(value), (cname, what)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in pairs.values())


def test_a_null_engine_is_refused_by_every_call_without_a_device():
    """Every call that takes an engine, with e = NULL and otherwise plausible arguments (addresses of host memory that no
    refusal reads): TKNN_E_ARG, said in the call's own name, on a machine with or without a GPU."""
    lib = _lib.load()
    assert set(cc.CALLS) == {name for name, (_, args) in _lib.SIGNATURES.items()
                             if name not in ("tknnCreate", "tknnDestroy") and not name.startswith("tknnDebug") and args}, "a call is missing"
    spare = ctypes.create_string_buffer(4096)
    addr = ctypes.addressof(spare)
    for fn in sorted(cc.CALLS):
        rc, message, info, _ = cc.call(lib, fn, None, addr, addr)
        assert rc == cc.E_ARG, (fn, rc, message)
        assert message.startswith(cc.SPEAKS_AS.get(fn, fn)), (fn, message)
        assert info is None or info == bytes([cc.INFO_FILL]) * len(info), fn  # (refused: info untouched)
    assert spare.raw == bytes(4096)


def test_calls_without_an_engine_refuse_bad_arguments():
    """tknnDestroy(NULL) does nothing; tknnCreate(NULL) and the two debug entry points with a NULL or out-of-range argument
    are refused before any device is looked for."""
    lib = _lib.load()
    lib.tknnDestroy(None)
    assert lib.tknnCreate(None) == cc.E_ARG
    assert lib.tknnLastError().decode().startswith("tknnCreate")
    spare = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(spare)
    good = dict(d_boxes=p, n=4, d_boxes_refit=None, mode=0, nodes=p, rope_node=p, rope_leaf=p, prim_id=p, sorted_boxes=p)
    for fault in (dict(d_boxes=None), dict(n=0), dict(n=-1), dict(n=cc.TOO_MANY), dict(mode=-1), dict(mode=3)):
        assert lib.tknnDebugBoxTree(*dict(good, **fault).values(), None) == cc.E_ARG, fault
        assert lib.tknnLastError().decode().startswith("tknnDebugBoxTree"), fault
    good = dict(d_q=p, d_r=p, n=4, d_lo=p, d_hi=p)
    for fault in (dict(d_q=None), dict(d_r=None), dict(d_lo=None), dict(d_hi=None), dict(n=-1)):
        assert lib.tknnDebugThresholds(*dict(good, **fault).values(), None) == cc.E_ARG, fault
        assert lib.tknnLastError().decode().startswith("tknnDebugThresholds"), fault
    assert spare.raw == bytes(4096)
