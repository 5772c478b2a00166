"""What the GPU tests of tknnRadiusKnn expect (tests/radius_knn_spec.py), checked on the CPU: that every case can catch what it
is meant to catch, and that the header, the ctypes mirrors and the signature table agree.  Runs without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import query_spec as qs  # noqa: E402
import radius_knn_spec as ks  # noqa: E402
import radius_spec as rs  # noqa: E402


def test_the_set_cases_are_exactly_the_sharp_combinations():
    """Every (set, factor, k) used on the GPU has a row shorter than k and a row longer than k; no sharp combination is left out."""
    sharp = tuple((name, f, k) for name in rs.SET_NAMES for f in rs.SET_FACTORS for k in ks.K_ALL if ks.set_case_is_sharp(name, f, k))
    assert ks.SET_CASES == sharp
    for name in {c[0] for c in ks.SET_CASES}:
        P, Q, _ = ks.knn_set(name)
        assert len(P) <= ks.MAX_N and len(Q) <= ks.MAX_M


def test_the_dense_case_is_sharp_at_every_k():
    P, Q, r, rows = ks.dense_rows()
    assert len(P) <= ks.MAX_N and len(Q) <= ks.MAX_M
    for k in ks.K_ALL:
        assert (rows["lengths"] < k).sum() >= 10 and (rows["lengths"] > k).sum() >= 10, k
    assert (rows["lengths"] == 0).any(), "empty rows: the whole row is padding"


def test_cut_rows_cuts_pads_and_skips():
    P, Q, r, rows = ks.dense_rows()
    want = ks.cut_rows(rows, 5)
    j = int(np.argmax(rows["lengths"] > 5))
    a = rows["offsets"][j]
    assert np.array_equal(want["idx"][j], rows["idx"][a:a + 5]) and want["counts"][j] == 5 and want["lengths"][j] == rows["lengths"][j]
    e = int(np.argmax(rows["lengths"] == 0))
    assert (want["idx"][e] == -1).all() and np.isinf(want["dist"][e]).all() and want["counts"][e] == 0
    skip = np.full(len(Q), -1, np.int64)
    skip[j] = rows["idx"][a]  # the row's nearest point
    cut = ks.cut_rows(rows, 5, skip)
    assert np.array_equal(cut["idx"][j], rows["idx"][a + 1:a + 6]) and cut["lengths"][j] == rows["lengths"][j] - 1
    assert np.array_equal(np.delete(cut["idx"], j, 0), np.delete(want["idx"], j, 0))
    # per-query radii: the rows of each radius, invalid radii empty
    radii = np.float32([0.2, np.nan, 0.1, 0.0, -1.0, np.inf] * 3)
    mixed = ks.knn_rows(P, Q[:18], 5, radii=radii)
    for t, r_t in enumerate(radii):
        if np.isfinite(r_t) and r_t > 0:
            one = ks.knn_rows(P, Q[t:t + 1], 5, radius=r_t)
            assert np.array_equal(mixed["idx"][t], one["idx"][0]) and mixed["counts"][t] == one["counts"][0]
        else:
            assert mixed["counts"][t] == 0 and (mixed["idx"][t] == -1).all()


def test_the_lattice_case_cuts_inside_ties():
    """Rows whose k-th and (k+1)-th candidates have bit-identical distances: the index decides which one the row holds."""
    P, Q, radii = rs.lattice_case()
    assert len(P) <= ks.MAX_N and len(Q) <= ks.MAX_M

    def tied_rows(t, k):
        rows = rs.radius_rows(P, Q, radii[t])
        n = 0
        for j in np.flatnonzero(rows["lengths"] > k):
            d = rows["dist"][rows["offsets"][j]:rows["offsets"][j + 1]].view(np.int32)
            n += int(d[k - 1] == d[k])
        return n, rows

    # r = the spacing: a node query has itself at 0 and up to six neighbours at exactly r; k = 3 and 6 cut inside them
    for k in (3, 6):
        n, rows = tied_rows(0, k)
        assert n >= 50, (k, n)
    assert (rows["lengths"] == 7).sum() >= 20 and 7 in ks.LATTICE_K, "L = k at k = 7"
    assert tied_rows(2, 1)[0] >= 100, "cell centres: eight corners at half the diagonal, k = 1 takes the lowest index"
    below = rs.radius_rows(P, Q, radii[1])
    assert (below["dist"] < rs.LATTICE_STEP).all() and below["offsets"][-1] < rows["offsets"][-1], "the float below the spacing excludes them"


def test_the_chunk_case_separates_each_length_from_the_next():
    P, Q, picks = rs.chunk_case()
    assert [L for L, _, _ in picks] == list(rs.CHUNK_LENGTHS) and len(P) <= ks.MAX_N and len(Q) <= ks.MAX_M
    for L, j, r in picks:
        d = np.sort(qs.distance32(P, Q[j]))
        assert (d <= r).sum() == L and d[L] > r, (L, j)
    lengths = [L for L, _, _ in picks]
    for k in ks.CHUNK_K:
        assert any(L < k for L in lengths) and k in lengths and any(L > k for L in lengths), k


def test_everything_in_reach_equals_the_exact_rows():
    P, Q = ks.uniform_case()
    want = ks.knn_rows(P, Q[:20], 10, radius=4.0)
    idx, dist = qs.exact_rows(P, Q[:20], 10)
    assert np.array_equal(want["idx"], idx) and np.array_equal(want["dist"].view(np.int32), dist.view(np.int32)) and (want["counts"] == 10).all()


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"TKNN_API[^;(]*?\b(tknn\w+)\s*\(", text))


def test_header_signatures_and_struct_layouts_agree(tmp_path):
    """tknnRadiusKnn is declared, bound with its signature, and the ctypes mirrors have the header's sizes and offsets (gcc, C99)."""
    from owlraytracing_amd import _lib

    assert "tknnRadiusKnn" in _declared("owlknn.h") and "tknnRadiusKnn" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["tknnRadiusKnn"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.POINTER(_lib.RadiusKnnOptions), ctypes.POINTER(_lib.RadiusKnnInfo), ctypes.c_void_p]
    pairs = {"tknnRadiusKnnOptions": _lib.RadiusKnnOptions, "tknnRadiusKnnInfo": _lib.RadiusKnnInfo}
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
    assert ctypes.sizeof(_lib.RadiusKnnOptions) == 64 and ctypes.sizeof(_lib.RadiusKnnInfo) == 56
    lib = _lib.load()
    assert hasattr(lib, "tknnRadiusKnn")
    for name in ("radius_knn.hip",):
        assert all(name in v for v in _lib._NOT_IN.values()), "the per-kernel profile records of team_* and db_* do not depend on it"
