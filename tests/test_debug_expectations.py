"""The test hooks tknnDebugPoison and tknnDebugTeamLanes without a GPU: include/owlknn_debug.h against owlraytracing_amd/_debug_lib.py
and the built library, the header as C99, and the refusals that need no device.  What the poison hook fills, and what calls make
of it, is tests/test_engine_state_gpu.py's; what the team helpers compute, tests/test_team_lanes_gpu.py's."""
import ctypes
import os
import re
import subprocess
import sys

from conftest import ROOT


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"TKNN_API[^;(]*?\b(tknn\w+)\s*\(", text))


def test_header_binding_and_constants_agree(tmp_path):
    """tknnDebugPoison and tknnDebugTeamLanes are declared in their own header, exported and bound with their signatures, nothing
    was added to owlknn.h or to _lib's table, and the binding's constants are the header's (gcc, C99)."""
    from owlraytracing_amd import _debug_lib, _lib

    assert _declared("owlknn_debug.h") == set(_debug_lib.SIGNATURES) == {"tknnDebugPoison", "tknnDebugTeamLanes"}
    assert "tknnDebugPoison" not in _declared("owlknn.h") and "tknnDebugPoison" not in _lib.SIGNATURES
    assert "tknnDebugTeamLanes" not in _declared("owlknn.h") and "tknnDebugTeamLanes" not in _lib.SIGNATURES
    lanes_res, lanes_args = _debug_lib.SIGNATURES["tknnDebugTeamLanes"]
    assert lanes_res is ctypes.c_int
    assert lanes_args == [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    res, args = _debug_lib.SIGNATURES["tknnDebugPoison"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]
    consts = {"TKNN_POISON_WORKSPACE": _debug_lib.POISON_WORKSPACE, "TKNN_POISON_COUNTERS": _debug_lib.POISON_COUNTERS, "TKNN_POISON_LISTS": _debug_lib.POISON_LISTS,
              "TKNN_POISON_SOLVE": _debug_lib.POISON_SOLVE, "TKNN_POISON_ALL": _debug_lib.POISON_ALL}
    lanes_ops = ["SORT16", "CLEAN16", "SORT16_U32", "SORTED_ROW", "MERGE", "KTH", "ROW_TIES", "STRADDLE", "FIRST_LEVEL", "REDUCE", "MOVES", "SORT16_3", "CLEAN16_3"]
    consts.update({"TKNN_LANES_" + op: getattr(_debug_lib, "LANES_" + op) for op in lanes_ops})
    consts.update({"TKNN_LANES_OPS": _debug_lib.LANES_OPS, "TKNN_LANES_MAX_TEAMS": _debug_lib.LANES_MAX_TEAMS})
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
    assert sorted(consts["TKNN_LANES_" + op] for op in lanes_ops) == list(range(consts["TKNN_LANES_OPS"])) and consts["TKNN_LANES_MAX_TEAMS"] == 1 << 20
    assert lib.tknnDebugTeamLanes.restype is ctypes.c_int and lib.tknnDebugTeamLanes.argtypes == lanes_args
    assert re.search(r"\bT tknnDebugTeamLanes$", exported, flags=re.M), "the library exports the symbol"
    diag = os.path.join(os.path.dirname(_lib.LIB_PATH), "libowl_mi355x_diag.so")
    if os.path.exists(diag):  # the harness rides in both libraries
        assert re.search(r"\bT tknnDebugTeamLanes$", subprocess.run(["nm", "-D", "--defined-only", diag], check=True, capture_output=True, text=True).stdout, flags=re.M)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import team_lanes_spec as ts

    assert [getattr(_debug_lib, "LANES_" + op) for op in ts.OP_NAMES] == [getattr(ts, op) for op in ts.OP_NAMES] == list(range(13)), "the specification's ops"
    assert ts.MAX_TEAMS == _debug_lib.LANES_MAX_TEAMS


def test_a_null_engine_is_refused_without_a_device():
    from owlraytracing_amd import _debug_lib

    lib = _debug_lib.load()
    filled = ctypes.c_int64(77)
    assert lib.tknnDebugPoison(None, _debug_lib.POISON_ALL, 0x5A, 0, ctypes.byref(filled), None) == -1
    assert lib.tknnLastError().decode().startswith("tknnDebugPoison: ") and "engine" in lib.tknnLastError().decode() and filled.value == 77


def test_team_lanes_refusals_need_no_device_and_come_in_order():
    """NULL pointers, then teams, then the op, then the variant: each refusal is TKNN_E_ARG, names its own reason even when
    everything after it is wrong too, and is decided before any device call (the pointers here are not device memory; nothing
    is read or written through them).  teams == 0 succeeds and launches nothing."""
    from owlraytracing_amd import _debug_lib

    lib = _debug_lib.load()
    words = (ctypes.c_uint32 * 64)(*([0xA5A5A5A5] * 64))
    p = ctypes.cast(words, ctypes.c_void_p)
    big = _debug_lib.LANES_MAX_TEAMS + 1
    cases = [  # (op, variant, in, out, teams), what the message must name
        ((99, 9, None, p, -1), "d_in"), ((99, 9, p, None, -1), "d_out"), ((99, 9, None, None, big), "d_in"),
        ((99, 9, p, p, -1), "teams"), ((99, 9, p, p, big), "teams"), ((_debug_lib.LANES_MERGE, 0, p, p, big), "teams"),
        ((99, 9, p, p, 4), "no such op"), ((-1, 1, p, p, 0), "no such op"), ((_debug_lib.LANES_OPS, 0, p, p, 4), "no such op"),
        ((_debug_lib.LANES_SORT16, 1, p, p, 4), "variant"), ((_debug_lib.LANES_MERGE, 0, p, p, 4), "variant"), ((_debug_lib.LANES_MERGE, 5, p, p, 0), "variant"),
        ((_debug_lib.LANES_KTH, 0, p, p, 4), "variant"), ((_debug_lib.LANES_ROW_TIES, 5, p, p, 4), "variant"), ((_debug_lib.LANES_MOVES, 64, p, p, 4), "variant"),
        ((_debug_lib.LANES_MOVES, -1, p, p, 4), "variant"), ((_debug_lib.LANES_CLEAN16_3, 2, p, p, 4), "variant"),
    ]
    for args, reason in cases:
        assert lib.tknnDebugTeamLanes(*args, None) == -1, args
        msg = lib.tknnLastError().decode()
        assert msg.startswith("tknnDebugTeamLanes: ") and reason in msg.split(": ", 1)[1], (args, msg)
        assert all(w == 0xA5A5A5A5 for w in words), args
    for op in range(_debug_lib.LANES_OPS):
        variant = 1 if op in (_debug_lib.LANES_MERGE, _debug_lib.LANES_KTH, _debug_lib.LANES_ROW_TIES) else 0
        assert lib.tknnDebugTeamLanes(op, variant, p, p, 0, None) == 0, op
    assert all(w == 0xA5A5A5A5 for w in words)
