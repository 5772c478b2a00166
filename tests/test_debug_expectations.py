"""The test hook tknnDebugPoison without a GPU: include/owlknn_debug.h against owlraytracing_amd/_debug_lib.py and the built library,
the header as C99, and the refusal that needs no device.  What the hook fills, and what calls make of it, is
tests/test_engine_state_gpu.py's."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"TKNN_API[^;(]*?\b(tknn\w+)\s*\(", text))


def test_header_binding_and_constants_agree(tmp_path):
    """tknnDebugPoison is declared in its own header, exported and bound with its signature, nothing was added to owlknn.h or to
    _lib's table, and the binding's constants are the header's (gcc, C99)."""
    from owlraytracing_amd import _debug_lib, _lib

    assert _declared("owlknn_debug.h") == set(_debug_lib.SIGNATURES) == {"tknnDebugPoison"}
    assert "tknnDebugPoison" not in _declared("owlknn.h") and "tknnDebugPoison" not in _lib.SIGNATURES
    res, args = _debug_lib.SIGNATURES["tknnDebugPoison"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]
    consts = {"TKNN_POISON_WORKSPACE": _debug_lib.POISON_WORKSPACE, "TKNN_POISON_COUNTERS": _debug_lib.POISON_COUNTERS, "TKNN_POISON_LISTS": _debug_lib.POISON_LISTS,
              "TKNN_POISON_SOLVE": _debug_lib.POISON_SOLVE, "TKNN_POISON_ALL": _debug_lib.POISON_ALL}
    lines = ["#include <stdio.h>", '#include "owlknn_debug.h"', "int main(void) {"]
    lines += ['  printf("%s %%ld\\n", (long)%s);' % (name, name) for name in consts]
    lines += ["  return 0;", "}"]
    src = tmp_path / "consts.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "consts"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert {line.split()[0]: int(line.split()[1]) for line in out.splitlines()} == consts
    assert consts["TKNN_POISON_ALL"] == 1 | 2 | 4 | 8
    lib = _debug_lib.load()
    assert lib is _lib.load() and lib.tknnDebugPoison.restype is ctypes.c_int and lib.tknnDebugPoison.argtypes == args
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT tknnDebugPoison$", exported, flags=re.M), "the library exports the symbol"


def test_a_null_engine_is_refused_without_a_device():
    from owlraytracing_amd import _debug_lib

    lib = _debug_lib.load()
    filled = ctypes.c_int64(77)
    assert lib.tknnDebugPoison(None, _debug_lib.POISON_ALL, 0x5A, 0, ctypes.byref(filled), None) == -1
    assert lib.tknnLastError().decode().startswith("tknnDebugPoison: ") and "engine" in lib.tknnLastError().decode() and filled.value == 77
