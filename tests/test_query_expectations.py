"""What the GPU tests of tknnQuery expect (tests/query_spec.py), checked on the CPU: the numpy restatement against the
append-one-query identity of the committed oracle, the sets against what each is for, the committed fixtures, and the
C-ABI's declaration, symbol and struct layout.  Runs without a GPU."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle  # noqa: E402
import query_spec as qs  # noqa: E402
from tile_sets import tie_order_needs_level  # noqa: E402

_sets = {}


def _set(name):
    if name not in _sets:
        _sets[name] = qs.make_set(name)
    return _sets[name]


def _identity(P, q, k, r0):
    o = oracle.trueknn_rows(np.concatenate([P, q[None]]), k, r0, np.array([len(P)], np.int32))
    level = o["rounds"] - 1
    return o["idx"][0], o["dist"][0], int(o["intersections"][0]) - (level + 1), level


@pytest.mark.parametrize("name", qs.SET_NAMES)
def test_spec_equals_the_oracle_identity(name):
    P, Q, r0 = _set(name)
    ks = (3, 5) if name == "tiny" else (3, 10)
    pick = np.sort(np.random.default_rng(7).choice(len(Q), min(len(Q), 120), replace=False))
    if name == "uniform":  # both kinds of queries
        pick = np.concatenate([pick[pick < len(Q) - qs.N_WIDE][:80], np.arange(len(Q) - 40, len(Q))])
    assert len(pick) >= 100 or name == "tiny"
    spec = qs.query_rows(P, Q[pick], ks, r0)
    for k in ks:
        bad = []
        for t, j in enumerate(pick):
            idx, dist, isect, level = _identity(P, Q[j], k, r0)
            s = spec[k]
            if not (np.array_equal(idx, s["idx"][t]) and np.array_equal(dist.view(np.int32), s["dist"][t].view(np.int32))
                    and isect == s["intersections"][t] and level == s["levels"][t]):
                bad.append(int(j))
        assert not bad, "%s k=%d: %d of %d rows differ from the oracle identity (first: query %d)" % (name, k, len(bad), len(pick), bad[0])


def test_lattice_rows_need_the_level_and_the_exact_pass():
    P, Q, r0 = _set("lattice")
    spec = qs.query_rows(P, Q, (3, 6, 10), r0)
    need = {k: int(tie_order_needs_level(spec[k]["idx"], spec[k]["dist"]).sum()) for k in (3, 6, 10)}
    assert need[10] > 0, "lattice k=10: no row whose reference order differs from (dist, index) order (k=3: %d, k=6: %d)" % (need[3], need[6])
    changed = {}
    for k in (3, 6, 10):
        s = spec[k]
        radius = np.float32(r0) * np.float32(2) ** s["levels"].astype(np.float32)
        beyond = int((s["dist"][:, -1] > radius).sum())
        want_idx, want_dist = qs.exact_rows(P, Q, k)
        differ = int(((want_idx != s["idx"]).any(axis=1) | (want_dist.view(np.int32) != s["dist"].view(np.int32)).any(axis=1)).sum())
        changed[k] = differ
        assert beyond > 0, "lattice k=%d: %d rows with d_k above the finishing radius" % (k, beyond)
    # (on a lattice a box that holds k points mostly holds the k nearest too: the rows the exact pass changes come with larger k)
    assert changed[10] > 0, "lattice: rows the exact pass changes: %s" % changed


def test_wide_queries_need_more_levels():
    P, Q, r0 = _set("uniform")
    pick = np.concatenate([np.arange(300), np.arange(len(Q) - 300, len(Q))])
    levels = qs.query_rows(P, Q[pick], (10,), r0)[10]["levels"] + 1
    inside, wide = float(levels[:300].mean()), float(levels[300:].mean())
    assert wide > inside + 1, "levels traced: %.2f inside the cube, %.2f in the cube twice as wide" % (inside, wide)


def test_sets_hit_what_they_are_for():
    P, Q, r0 = _set("copies")
    s = qs.query_rows(P, Q[:200], (2,), r0)[2]
    assert (s["dist"][:, 0] == 0).all(), "copies: neighbour 0 is the point itself at distance 0"
    P, Q, r0 = _set("clustered")
    s = qs.query_rows(P, Q[:200], (10,), r0)[10]
    # a box that finishes among evenly spread points holds k .. 8 k candidates (one doubling); ten times k and more is a cluster swallowed whole
    assert np.median(s["intersections"]) >= 100 and s["levels"].mean() > 4, "clustered: median %d candidates per query at k = 10, %.1f levels" % (
        np.median(s["intersections"]), s["levels"].mean())
    P, Q, r0 = _set("tiny")
    s = qs.query_rows(P, Q, (5,), r0)[5]
    assert (s["levels"] >= 0).all() and all(sorted(row) == [0, 1, 2, 3, 4] for row in s["idx"]), "tiny: n = k = 5 finishes with every point"
    P, Q, r0 = _set("planar")
    assert (P[:, 2] == 0).all() and (Q[:800, 2] == 0).all() and (Q[800:, 2] != 0).any()
    P, Q, r0 = _set("duplicates")
    s = qs.query_rows(P, Q[-200:], (3,), r0)[3]
    assert (s["dist"][:, 0] == 0).all() and (s["dist"][:, 1] == 0).any(), "duplicates: repeated points are several neighbours at distance 0"


def test_nan_and_unfinished_in_the_spec():
    P, Q, r0 = _set("lattice")
    Qn = Q[:4].copy()
    Qn[1, 0] = np.nan
    s = qs.query_rows(P, Qn, (4,), r0, max_rounds=5)[4]
    assert s["levels"][1] == -1 and s["unfinished"] == 1 and s["rounds"] == 5 and s["total_active_rounds"] == 5 + int((s["levels"][[0, 2, 3]] + 1).sum())


def test_committed_fixtures_equal_the_spec():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "queries", "*.npz")))
    assert len(files) == 3
    largest = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    for path in files:
        assert os.path.getsize(path) <= largest, path
        with np.load(path) as z:
            g = {name: z[name] for name in z.files}
        k = int(g["k"])
        s = qs.query_rows(g["points"], g["queries"], (k,), float(g["start_radius"]))[k]
        assert np.array_equal(s["idx"], g["idx"]) and np.array_equal(s["dist"].view(np.int32), g["dist"].view(np.int32)), path
        assert np.array_equal(s["intersections"], g["intersections"]) and np.array_equal(s["levels"], g["levels"]), path


def test_cabi_declares_and_exports_tknnQuery(tmp_path):
    """The header declares tknnQuery, the library has the symbol, tknnQueryOptions has the layout of its ctypes mirror."""
    from owlraytracing_amd import _lib

    header = open(os.path.join(ROOT, "include", "owlknn.h")).read()
    assert re.search(r"TKNN_API\s+int\s+tknnQuery\s*\(", header) and "TKNN_KERNEL_QUERY = 4" in header
    assert "tknnQuery" in _lib.SIGNATURES and _lib.KERNEL_QUERY == 4
    assert hasattr(_lib.load(), "tknnQuery")
    cls = _lib.QueryOptions
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(tknnQueryOptions));']
    for field, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(tknnQueryOptions, %s));' % (field, field))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cls._fields_) + 1
    for line in out:
        what, value = line.split()
        if what == "size":
            assert ctypes.sizeof(cls) == int(value)
        else:
            assert getattr(cls, what).offset == int(value), what
