"""What the GPU tests of tknnDbscanQuery expect (tests/dbscan_query_spec.py), checked on the CPU: the numpy restatement with
Q = P against the committed oracle's clustering, the slabs set against what it is for, the C-ABI's declaration, symbol and
struct layout, and the call's workspace layout (db_workspace.h) in a stand-alone host program.  Runs without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import dbscan_query_spec as ds  # noqa: E402


@pytest.mark.parametrize("name", ["slabs", "mixture"])
def test_spec_with_the_set_as_queries_equals_the_oracle(name):
    c = ds.cases(name)[0]
    ref = c["oracle"]
    labels, counts = ds.query_labels(c["P"], c["core_label"], c["eps"], c["P"])
    assert np.array_equal(labels, ref["labels"]), "%d rows differ" % int((labels != ref["labels"]).sum())
    assert np.array_equal(counts, ref["counts"])
    assert np.array_equal(counts >= c["min_pts"], ref["core"])


def test_slabs_are_what_they_claim():
    c = ds.cases("slabs")[0]
    assert c["oracle"]["clusters"] == 3
    reached = ds.clusters_reached(c["P"], c["core_label"], c["eps"], c["Q"])
    several = reached > 1
    nearest = ds.nearest_core_label(c["P"], c["core_label"], c["eps"], c["Q"])
    not_nearest = several & (nearest != c["labels"])
    noise = c["labels"] < 0
    print("slabs: %d queries reach more than one cluster, %d of them with a nearest core point of another label, %d noise" % (
        several.sum(), not_nearest.sum(), noise.sum()))
    assert several.sum() >= 100
    assert not_nearest.sum() >= 50
    assert noise.sum() >= 100
    assert (c["counts"][-300:] >= 1).all(), "a copy of a point of the set has that point as a neighbour"


def test_sets_hold_the_edge_cases():
    tiny = {c["name"]: c for c in ds.cases("tiny")}
    assert [len(tiny[k]["P"]) for k in ("n1_minpts1", "n2_minpts1", "n5_minpts2")] == [1, 2, 5]
    assert (tiny["no_core_point"]["core_label"] < 0).all() and (tiny["no_core_point"]["labels"] == -1).all()
    assert (tiny["no_core_point"]["counts"] > 0).any(), "neighbours, but no core point among them"
    assert tiny["duplicates64"]["counts"].max() == 64 and (tiny["n1_minpts1"]["labels"] == 0).any()
    nan = ds.cases("nan")[0]
    assert np.isnan(nan["P"]).any(axis=1).sum() == 7
    qn = np.isnan(nan["Q"]).any(axis=1)
    assert qn.sum() == 5 and (nan["labels"][qn] == -1).all() and (nan["counts"][qn] == 0).all()
    assert (nan["labels"] >= 0).sum() > 50 and (nan["labels"] < 0).sum() > 5
    edges = ds.cases("edges")
    assert tuple(len(c["Q"]) for c in edges) == ds.EDGE_M
    assert max(float(np.abs(c["Q"]).max()) for c in edges) >= 10
    assert all((c["labels"] >= 0).any() for c in edges if len(c["Q"]) >= 63)


def test_cabi_declares_and_exports_tknnDbscanQuery(tmp_path):
    """The header declares tknnDbscanQuery, the library has the symbol, tknnDbscanQueryOptions has the layout of its ctypes mirror."""
    from owlraytracing_amd import _lib

    header = open(os.path.join(ROOT, "include", "owlknn.h")).read()
    assert re.search(r"TKNN_API\s+int\s+tknnDbscanQuery\s*\(", header)
    assert "tknnDbscanQuery" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "tknnDbscanQuery")
    cls = _lib.DbscanQueryOptions
    assert [f for f, _ in cls._fields_] == ["d_queries", "m", "eps", "reserved_", "d_core_label", "d_labels", "d_counts"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(tknnDbscanQueryOptions));']
    for field, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(tknnDbscanQueryOptions, %s));' % (field, field))
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


# The query call's scratch (DbQueryWs): a stand-alone host program with its own main, built with the address and undefined-
# behaviour sanitizers, prints every region's offset and asserts what the kernels rely on; the lines it prints are checked
# once more here against the bytes each region has to hold.
QUERY_REGIONS = ["pos", "next_core", "block_places", "core_sorted", "codes", "codes_sorted", "order_in", "order"]
LAYOUT_N = [1, 255, 256, 257, 10**7]
LAYOUT_M = [1, 63, 257, 10**7]
_PROGRAM = r"""
#include <assert.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "db_workspace.h"
using namespace owlmi;
int main() {
  const size_t ns[] = {1, 255, 256, 257, 10000000}, ms[] = {1, 63, 257, 10000000};
  for (size_t n : ns)
    for (size_t m : ms) {
      const DbQueryWs w = DbQueryWs::of(n, m);
      const size_t at[] = {w.pos, w.next_core, w.block_places, w.core_sorted, w.codes, w.codes_sorted, w.order_in, w.order};
      const size_t need[] = {(n + 1) * 4, (n + 1) * 4, ((n + kDbBlock - 1) / kDbBlock) * 8, n, m * 4, m * 4, m * 4, m * 4};
      std::vector<std::pair<size_t, size_t>> spans;
      printf("n %zu m %zu end %zu", n, m, w.end);
      for (int i = 0; i < 8; i++) {
        printf(" %zu", at[i]);
        assert(at[i] % kDbRegionAlign == 0);
        assert(at[i] + need[i] <= w.end);
        spans.push_back({at[i], at[i] + need[i]});
      }
      printf("\n");
      std::sort(spans.begin(), spans.end());
      for (size_t i = 0; i + 1 < spans.size(); i++) assert(spans[i].second <= spans[i + 1].first);
      assert(w.end == DbQueryWs::bytes(n, m));
      assert(db_round_up(w.end, kDbScanAlign) % kDbScanAlign == 0 && db_round_up(w.end, kDbScanAlign) - w.end < kDbScanAlign);
    }
  return 0;
}
"""


def test_query_workspace_layout_in_a_sanitized_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "query_layout.cpp", tmp_path / "query_layout"
    src.write_text(_PROGRAM)
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "owlraytracing_amd", "csrc"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(LAYOUT_N) * len(LAYOUT_M)
    seen = set()
    for line in lines:
        w = line.split()
        n, m, end = int(w[1]), int(w[3]), int(w[5])
        seen.add((n, m))
        at = dict(zip(QUERY_REGIONS, (int(x) for x in w[6:])))
        assert len(at) == len(QUERY_REGIONS)
        needs = {"pos": 4 * (n + 1), "next_core": 4 * (n + 1), "block_places": 8 * ((n + 255) // 256), "core_sorted": n,
                 "codes": 4 * m, "codes_sorted": 4 * m, "order_in": 4 * m, "order": 4 * m}
        spans = sorted((at[k], at[k] + needs[k], k) for k in needs)
        for (lo, hi, k), (lo2, _, k2) in zip(spans, spans[1:]):
            assert hi <= lo2, "%s runs into %s" % (k, k2)
        for lo, hi, k in spans:
            assert lo % 16 == 0 and hi <= end, k
        assert end <= 9 * n + 16 * m + 16 * 12 + 8 * (n // 256 + 2)  # nothing but the regions and their padding
    assert seen == {(n, m) for n in LAYOUT_N for m in LAYOUT_M}
