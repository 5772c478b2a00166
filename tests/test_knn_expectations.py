"""What the GPU tests of tknnKnn expect (tests/knn_spec.py), checked on the CPU: the spec against tknnRadiusKnn's at the largest
finite radius, that every case can catch what it is meant to catch, and that the header include/owlknn_knn.h, the ctypes records
of owlraytracing_amd/_knn_lib.py and the library agree.  Runs without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_spec as kn  # noqa: E402
import radius_knn_spec as rk  # noqa: E402

FLT_MAX = np.finfo(np.float32).max
ARG = -1


def _equal(a, b, what):
    assert np.array_equal(a["idx"], b["idx"]), what
    assert np.array_equal(a["dist"].view(np.int32), b["dist"].view(np.int32)), what
    assert np.array_equal(a["counts"], b["counts"]), what


@pytest.mark.parametrize("name", kn.SET_NAMES)
def test_the_spec_is_radius_knn_at_the_largest_finite_radius(name):
    P, Q, rows = kn.set_rows(name)
    assert len(P) <= rk.MAX_N and len(Q) <= rk.MAX_M
    for k in (1, 17, 64):
        _equal(kn.cut(rows, k), rk.knn_rows(P, Q, k, radius=FLT_MAX), "%s k=%d" % (name, k))
    assert (rows["counts"] == kn.K_MAX).all()


def test_the_spec_is_radius_knn_in_the_other_cases_too():
    P, Q = kn.nan_case()
    got = kn.knn_rows(P, Q, 20)
    _equal(got, rk.knn_rows(P, Q, 20, radius=FLT_MAX), "nan")
    nan_q, nan_p = np.isnan(Q).any(axis=1), np.flatnonzero(np.isnan(P).any(axis=1))
    assert nan_q.sum() == 5 and (got["counts"][nan_q] == 0).all() and (got["counts"][~nan_q] == 20).all()
    assert len(nan_p) == 23 and not np.isin(got["idx"], nan_p).any()
    P, Q = kn.far_case()
    _equal(kn.knn_rows(P, Q, 33), rk.knn_rows(P, Q, 33, radius=FLT_MAX), "far")
    for n in kn.TINY_N:
        P, Q, ks = kn.tiny_case(n)
        assert min(ks) < n or n == 1
        assert (n in ks and max(ks) > n) or n > kn.K_MAX  # (65 points: k = 64 is the eligible count of a point's own row)
        for k in ks:
            _equal(kn.knn_rows(P, Q, k), rk.knn_rows(P, Q, k, radius=FLT_MAX), "tiny n=%d k=%d" % (n, k))
    # skips and ids: self mode is the external call with every point skipped in its own row
    P = rk.knn_set("duplicates")[0][:600]
    ids = (np.random.default_rng(76).permutation(len(P)) * 3 + 1_000_000).astype(np.int32)
    _equal(kn.self_rows(P, 5), rk.knn_rows(P, P, 5, radius=FLT_MAX, skip=np.arange(len(P))), "self")
    _equal(kn.self_rows(P, 5, ids=ids), rk.knn_rows(P, P, 5, radius=FLT_MAX, skip=ids, ids=ids), "self, by id")
    own = kn.self_rows(P, 5)
    assert not (own["idx"] == np.arange(len(P))[:, None]).any() and (own["dist"][:, 0] == 0).sum() >= 20, "a coinciding duplicate stays"
    # an overflowing distance is no neighbour's
    big = np.float32([[3e38, 0, 0], [-3e38, 0, 0], [1, 1, 1]])
    rows = kn.knn_rows(big, np.float32([[-3e38, 0, 0], [0, 0, 0]]), 3)
    assert rows["counts"].tolist() == [1, 1] and rows["idx"][0].tolist() == [1, -1, -1] and rows["idx"][1].tolist() == [2, -1, -1]


def test_cut_pads_and_counts():
    P, Q, ks = kn.tiny_case(17)
    rows = kn.knn_rows(P, Q, kn.K_MAX)
    assert (rows["counts"] == 17).all() and (rows["idx"][:, 17:] == -1).all() and np.isposinf(rows["dist"][:, 17:]).all()
    for k in ks:
        _equal(kn.cut(rows, k), kn.knn_rows(P, Q, k), k)


def test_the_lattice_case_has_ties_at_the_kth_place_at_every_k():
    """Rows whose k-th and (k+1)-th entries have bit-identical distances: the index decides which one the row holds."""
    P, Q = kn.lattice_case()
    assert len(P) <= rk.MAX_N and len(Q) <= rk.MAX_M
    d = kn.knn_rows(P, Q, max(rk.LATTICE_K) + 1)["dist"].view(np.int32)
    for k in rk.LATTICE_K:
        assert (d[:, k - 1] == d[:, k]).sum() >= 20, k
    own = kn.self_rows(P, max(rk.LATTICE_K) + 1)["dist"].view(np.int32)
    for k in (1, 3):  # self mode: the six neighbours at the spacing are entries 1 .. 6 of an inner node
        assert (own[:, k - 1] == own[:, k]).sum() >= 20, k


def test_the_duplicates_case_has_a_kth_distance_of_zero_at_every_k():
    P, Q = kn.duplicates_case()
    assert (np.all(P == Q[0], axis=1)).sum() == kn.DUPLICATE_COPIES > max(kn.DUPLICATE_K)
    for k in kn.DUPLICATE_K:
        rows = kn.knn_rows(P, Q, k)
        assert rows["dist"][0, k - 1] == 0 and (rows["dist"][1:, k - 1] > 0).all(), k
    own = kn.self_rows(P, 64)
    assert (own["dist"][:, 63] == 0).sum() == kn.DUPLICATE_COPIES, "self mode: each copy has 69 others at distance 0"


def test_the_far_case_is_far_and_between():
    P, Q = kn.far_case()
    width = (P.max(0) - P.min(0)).max()
    d1 = kn.knn_rows(P, Q, 1)["dist"][:, 0]
    assert (d1[:8] > 9 * width).all(), "ten scene widths outside"
    rows = kn.knn_rows(P, Q[8:9], 64)
    low = (P[rows["idx"][0]] < 0.5).all(axis=1)
    assert 0 < low.sum() < 64, "the midpoint's row holds points of both clusters"


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"TKNN_API[^;(]*?\b(tknn\w+)\s*\(", text))


def test_header_binding_and_struct_layouts_agree(tmp_path):
    """tknnKnn is declared in its own header, exported and bound with its signature, nothing was added to owlknn.h or to _lib's
    tables, and the ctypes records have the header's sizes and offsets (gcc, C99)."""
    from owlraytracing_amd import _knn_lib, _lib

    assert _declared("owlknn_knn.h") == set(_knn_lib.SIGNATURES) == {"tknnKnn"}
    assert "tknnKnn" not in _declared("owlknn.h") and "tknnKnn" not in _lib.SIGNATURES and not hasattr(_lib, "KnnOptions")
    res, args = _knn_lib.SIGNATURES["tknnKnn"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.POINTER(_knn_lib.KnnOptions), ctypes.POINTER(_knn_lib.KnnInfo), ctypes.c_void_p]
    pairs = {"tknnKnnOptions": _knn_lib.KnnOptions, "tknnKnnInfo": _knn_lib.KnnInfo}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn_knn.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
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
    assert ctypes.sizeof(_knn_lib.KnnOptions) == 56 and ctypes.sizeof(_knn_lib.KnnInfo) == 72
    lib = _knn_lib.load()
    assert lib is _lib.load() and lib.tknnKnn.restype is ctypes.c_int and lib.tknnKnn.argtypes == args
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT tknnKnn$", exported, flags=re.M), "the library exports the symbol"
    for name in ("knn_seed.hip",):
        assert all(name in v for v in _lib._NOT_IN.values()), "the per-kernel profile records of team_* and db_* do not depend on it"


def test_a_null_engine_is_refused_without_a_device():
    from owlraytracing_amd import _knn_lib, _lib

    lib = _knn_lib.load()
    o, info = _knn_lib.KnnOptions(), _knn_lib.KnnInfo()
    info.total = 99
    assert lib.tknnKnn(None, ctypes.byref(o), ctypes.byref(info), None) == ARG
    text = lib.tknnLastError().decode()
    assert text.startswith("tknnKnn") and "engine" in text and info.total == 99, text
