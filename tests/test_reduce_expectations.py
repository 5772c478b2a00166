"""tests/reduce_spec.py against itself and against the C ABI, without a GPU: the tolerance is not too tight for an honest fp32
summation in any of three orders, the rows left out of the normalised comparison stay under their cap, the spec's rows are
radius_spec's, and include/owlknn_reduce.h, owlraytracing_amd/_reduce_lib.py and the built library agree."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import radius_spec as rs  # noqa: E402
import reduce_spec as rd  # noqa: E402

# the sets whose rows are short enough to be summed row by row in Python, with the radius classes of each
SMALL_SETS = ("n1", "n15", "n16", "n17", "n1025", "planar", "scale_up", "dup_own", "nan", "ids", "batched")
CHANNELS = (0, 1, 5, 14)  # a mass-like column, a coordinate-like one, a large and a small one


def weight32(weight, d2, d, r, h):
    """The weights as an fp32 evaluation of the header's formulas gives them, every operation rounded on its own."""
    f = np.float32
    d2, d = d2.astype(f), d.astype(f)
    if weight == "one":
        return np.ones_like(d2)
    k = rd.constants(weight, r, h)
    if weight == "gauss":
        return np.exp((d2 * k).astype(f)).astype(f)  # (numpy's float32 exp is within one ulp)
    if weight == "epanechnikov":
        return np.maximum(f(0), f(1) - d2 * k)
    s = d * k
    s2, t = s * s, f(2) - s
    return np.where(s <= 1, (f(1) - f(1.5) * s2) + f(0.75) * (s2 * s), np.maximum(f(0), f(0.25) * ((t * t) * t))).astype(f)


def pairwise32(t):
    t = t.astype(np.float32)
    while len(t) > 1:
        if len(t) % 2:
            t = np.concatenate([t, np.zeros(1, np.float32)])
        t = t[0::2] + t[1::2]
    return t[0] if len(t) else np.float32(0)


def running32(t):
    return np.add.accumulate(t.astype(np.float32), dtype=np.float32)[-1] if len(t) else np.float32(0)


@pytest.mark.parametrize("weight", rd.WEIGHTS)
@pytest.mark.parametrize("name", SMALL_SETS)
def test_the_bound_admits_fp32_summation_in_three_orders(name, weight):
    c = rd.case(name)
    for label, r in c["radii"].items():
        h = rd.bandwidth(r)
        mem = rd.rows_of(name, label, "ext")
        want = rd.sums(mem, c["values"][:, list(CHANNELS)], weight, r, h)
        tol = rd.tolerances(want, weight, r, h)
        w32 = weight32(weight, mem["d2"], mem["d"], r, h)
        assert (np.abs(w32.astype(np.float64) - want["w"]) <= rd.c_k(weight, r, h) * rd.U + 1e-37).all(), "c_K covers the fp32 weight"
        rows = np.flatnonzero(mem["lengths"])[:: max(1, len(mem["lengths"]) // 40)]  # forty rows of the case, spread
        for j in rows:
            lo, hi = mem["offsets"][j], mem["offsets"][j + 1]
            w = w32[lo:hi]
            for order in (slice(None), slice(None, None, -1)):
                for total in (running32, pairwise32):
                    assert abs(float(total(w[order])) - want["wsum"][j]) <= tol["wsum"][j], (label, j, "wsum")
                    for col, ch in enumerate(CHANNELS):
                        t = (w * c["values"][mem["idx"][lo:hi], ch]).astype(np.float32)
                        assert abs(float(total(t[order])) - want["out"][j, col]) <= tol["out"][j, col], (label, j, ch)


@pytest.mark.parametrize("name", rd.SET_NAMES)
def test_rim_rows_stay_under_the_cap_and_counts_are_radius_spec(name):
    c = rd.case(name)
    small = name in SMALL_SETS
    for label, r in c["radii"].items():
        for mode in rd.modes_of(name):
            mem = rd.rows_of(name, label, mode)
            if mode == "ext" and small:
                assert np.array_equal(mem["lengths"], rs.radius_rows(c["P"], c["Q"], r)["lengths"]), "the rows are radius_spec's"
            for weight in rd.WEIGHTS:
                w = rd.weights64(weight, mem["d2"], mem["d"], r, rd.bandwidth(r))
                assert (w <= 1).all() and (w >= 0).all()
                W = np.bincount(np.repeat(np.arange(len(mem["lengths"])), mem["lengths"]), weights=w, minlength=len(mem["lengths"]))
                rim = (mem["lengths"] > 0) & (W < rd.RIM_SHARE * mem["lengths"])
                assert rim.sum() <= rd.RIM_CAP * len(rim), (label, mode, weight, int(rim.sum()))


def test_rows_against_radius_spec_on_the_shared_cases():
    P, Q, picks, _ = rd.chunk_case()
    for L, j, r in picks:
        mem = rd.members(P, Q, r)
        rows = rs.radius_rows(P, Q, r)
        assert mem["lengths"][j] == L and np.array_equal(mem["lengths"], rows["lengths"])
        for q in range(0, len(Q), 9):
            mine = mem["idx"][mem["offsets"][q]:mem["offsets"][q + 1]]
            assert np.array_equal(np.sort(rows["idx"][rows["offsets"][q]:rows["offsets"][q + 1]]), mine)
    P, Q, radii, _ = rd.lattice_case()
    for r in radii:
        assert np.array_equal(rd.members(P, Q, r)["lengths"], rs.radius_rows(P, Q, r)["lengths"])
    # the set's own points: the point itself is a neighbour unless skipped; a coinciding duplicate stays
    c = rd.case("dup_own")
    r = c["radii"]["mid"]
    own, skip = rd.members(c["P"], None, r), rd.members(c["P"], None, r, skip_self=True)
    assert np.array_equal(own["lengths"], rs.radius_rows(c["P"], c["P"], r)["lengths"]) and np.array_equal(own["lengths"] - 1, skip["lengths"])
    tiny = rd.members(c["P"], None, np.float32(1e-6), skip_self=True)
    assert 0 < (tiny["lengths"] > 0).sum() < len(c["P"]) and (tiny["d2"] == 0).all()


def test_weights_by_hand():
    r, h = np.float32(2.0), np.float32(0.5)
    d = np.float32([0.0, 0.5, 1.0, 1.5, 2.0])
    d2 = d * d
    assert rd.constants("gauss", r, h) == np.float32(-2.0) and rd.constants("epanechnikov", r) == np.float32(0.25) and rd.constants("cubic_spline", r) == 1
    assert np.allclose(rd.weights64("gauss", d2, d, r, h), np.exp(-2.0 * d2.astype(np.float64)), rtol=0, atol=1e-15)
    assert rd.weights64("epanechnikov", d2, d, r).tolist() == [1.0, 0.9375, 0.75, 0.4375, 0.0]
    assert rd.weights64("cubic_spline", d2, d, r).tolist() == [1.0, 1 - 1.5 * 0.25 + 0.75 * 0.125, 0.25, 0.25 * 0.125, 0.0]
    assert rd.weights64("one", d2, d, r).tolist() == [1.0] * 5
    assert rd.c_k("one", r) == 0 and rd.c_k("epanechnikov", r) == 16 and rd.c_k("gauss", r, h) == 2 * (8 + 2)


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"TKNN_API[^;(]*?\b(tknn\w+)\s*\(", text))


def test_header_binding_and_struct_layouts_agree(tmp_path):
    """tknnRadiusReduce is declared in its own header, exported and bound with its signature, nothing was added to owlknn.h or to
    _lib's tables, and the ctypes records have the header's sizes and offsets (gcc, C99)."""
    from owlraytracing_amd import _lib, _reduce_lib

    assert _declared("owlknn_reduce.h") == set(_reduce_lib.SIGNATURES) == {"tknnRadiusReduce"}
    assert "tknnRadiusReduce" not in _declared("owlknn.h") and "tknnRadiusReduce" not in _lib.SIGNATURES
    res, args = _reduce_lib.SIGNATURES["tknnRadiusReduce"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.POINTER(_reduce_lib.RadiusReduceOptions), ctypes.POINTER(_reduce_lib.RadiusReduceInfo), ctypes.c_void_p]
    pairs = {"tknnRadiusReduceOptions": _reduce_lib.RadiusReduceOptions, "tknnRadiusReduceInfo": _reduce_lib.RadiusReduceInfo}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn_reduce.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    consts = {"TKNN_REDUCE_NORMALIZE": _reduce_lib.REDUCE_NORMALIZE, "TKNN_REDUCE_SKIP_SELF": _reduce_lib.REDUCE_SKIP_SELF, "TKNN_W_ONE": _reduce_lib.W_ONE,
              "TKNN_W_GAUSS": _reduce_lib.W_GAUSS, "TKNN_W_EPANECHNIKOV": _reduce_lib.W_EPANECHNIKOV, "TKNN_W_CUBIC_SPLINE": _reduce_lib.W_CUBIC_SPLINE,
              "TKNN_REDUCE_MAX_CHANNELS": _reduce_lib.MAX_CHANNELS}
    for cname in consts:
        lines.append('  printf("const %s %%ld\\n", (long)%s);' % (cname, cname))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        cname, what, value = line.split()
        if cname == "const":
            assert consts[what] == int(value), what
        elif what == "size":
            assert ctypes.sizeof(pairs[cname]) == int(value), cname
        else:
            assert getattr(pairs[cname], what).offset == int(value), (cname, what)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in pairs.values()) + len(consts)
    assert ctypes.sizeof(_reduce_lib.RadiusReduceOptions) == 72 and ctypes.sizeof(_reduce_lib.RadiusReduceInfo) == 56
    assert set(_reduce_lib.WEIGHTS) == set(rd.WEIGHTS)
    lib = _reduce_lib.load()
    assert lib is _lib.load() and lib.tknnRadiusReduce.restype is ctypes.c_int and lib.tknnRadiusReduce.argtypes == args
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT tknnRadiusReduce$", exported, flags=re.M), "the library exports the symbol"


def test_a_null_engine_is_refused_without_a_device():
    from owlraytracing_amd import _reduce_lib

    lib = _reduce_lib.load()
    o, info = _reduce_lib.RadiusReduceOptions(), _reduce_lib.RadiusReduceInfo()
    info.total = 77
    assert lib.tknnRadiusReduce(None, ctypes.byref(o), ctypes.byref(info), None) == -1
    assert lib.tknnLastError().decode().startswith("tknnRadiusReduce: ") and "engine" in lib.tknnLastError().decode() and info.total == 77
