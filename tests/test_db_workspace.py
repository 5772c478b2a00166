"""RT-DBSCAN's scratch layouts (owlraytracing_amd/csrc/db_workspace.h), compiled for the host: regions that are not declared
aliases do not overlap, every region lies inside bytes() and holds what the kernels put there (restated here), every region
begins at a multiple of 16 bytes (the kernels move four slots' words at once), and neither layout needs more room than the
hand-written arithmetic it replaced -- the 100 M-point run fits the device with the full clustering's workspace as it was."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 255, 256, 257, 10**7, 10**8]

CLUSTER = ["parent", "roots", "ranks", "next_core", "core_sorted", "min_row", "not_core", "border_lists", "uni", "block_places", "pk_diag"]
CLUSTER_ALIASES = {"groups": "roots", "is_root": "roots", "by_slot": "roots", "pos": "ranks", "group_at": "ranks", "uni_leaf": "ranks", "rank": "ranks"}
PROBE = ["near_node", "pos", "next_core", "block_places", "core_sorted", "noise"]

_SHIM = r"""
#include "db_workspace.h"
using namespace owlmi;
typedef unsigned long long u64;
extern "C" {
u64 cluster_layout(u64 n, int diag, u64 *at, u64 *alias) {
  const DbClusterWs w = DbClusterWs::of(n, diag != 0);
  const size_t r[] = {w.parent, w.roots, w.ranks, w.next_core, w.core_sorted, w.min_row, w.not_core, w.border_lists, w.uni, w.block_places, w.pk_diag};
  for (int i = 0; i < 11; i++) at[i] = r[i];
  const size_t a[] = {w.groups(), w.is_root(), w.by_slot(), w.pos(), w.group_at(), w.uni_leaf(), w.rank()};
  for (int i = 0; i < 7; i++) alias[i] = a[i];
  return w.end == DbClusterWs::bytes(n, diag != 0) ? w.end : ~0ull;
}
u64 probe_layout(u64 n, u64 *at) {
  const DbProbeWs w = DbProbeWs::of(n);
  const size_t r[] = {w.near_node, w.pos, w.next_core, w.block_places, w.core_sorted, w.noise};
  for (int i = 0; i < 6; i++) at[i] = r[i];
  return w.end == DbProbeWs::bytes(n) ? w.end : ~0ull;
}
u64 region_align() { return kDbRegionAlign; }
u64 block() { return kDbBlock; }
u64 scan_offset(u64 bytes) { return db_round_up(bytes, kDbScanAlign); }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("db_workspace")
    src, so = d / "shim.cpp", d / "libdbworkspace.so"
    src.write_text(_SHIM)
    subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "owlraytracing_amd", "csrc"),
                    str(src), "-o", str(so)], check=True, capture_output=True, text=True)
    so = ctypes.CDLL(str(so))
    for f in (so.cluster_layout, so.probe_layout, so.region_align, so.block, so.scan_offset):
        f.restype = ctypes.c_uint64
    return so


def _words(n):
    return 4 * n


def _block_places(n):
    return 2 * 4 * ((n + 255) // 256)  # a count and a place per workgroup of 256 slots


def _cluster_needs(n, diag):
    """bytes the kernels of the full clustering read or write in each region"""
    return {"parent": _words(n), "roots": _words(n), "ranks": _words(n + 1), "next_core": _words(n + 1), "core_sorted": n, "min_row": _words(n),
            "not_core": _words(n), "border_lists": _words(n), "uni": _words(n), "block_places": _block_places(n),
            "pk_diag": 16 * (n // 64 + 1) if diag else 0}


def _probe_needs(n):
    return {"near_node": _words(n), "pos": _words(n + 1), "next_core": _words(n + 1), "block_places": _block_places(n), "core_sorted": n, "noise": n}


def _check_regions(at, needs, total, align):
    spans = sorted((at[k], at[k] + needs[k], k) for k in needs)
    for (lo, hi, k), (lo2, _, k2) in zip(spans, spans[1:]):
        assert hi <= lo2, "%s runs into %s" % (k, k2)
    for lo, hi, k in spans:
        assert hi <= total, "%s ends behind bytes()" % k
        assert lo % align == 0, "%s is not aligned" % k


def _parent_cluster_bytes(n, diag):
    """the arithmetic Engine::dbscan did by hand before the header: (min_row_at + 16 n + block_places_bytes [+ 16 (n / 64 + 1)] + 255) / 256 * 256"""
    n = np.uint64(n)
    u = np.uint64
    min_row_at = (n * u(17) + u(8) + u(15)) // u(16) * u(16)
    block_places_bytes = ((n // u(256) + u(2)) * u(8) + u(15)) // u(16) * u(16)
    diag_bytes = (n // u(64) + u(1)) * u(16) if diag else u(0)
    return int((min_row_at + n * u(16) + block_places_bytes + diag_bytes + u(255)) // u(256) * u(256))


def _parent_probe_bytes(n):
    return (22 * n + 32 + 255) // 256 * 256


@pytest.mark.parametrize("diag", [False, True], ids=["plain", "diag_records"])
@pytest.mark.parametrize("n", SIZES)
def test_cluster_layout(lib, n, diag):
    at, alias = (ctypes.c_uint64 * len(CLUSTER))(), (ctypes.c_uint64 * len(CLUSTER_ALIASES))()
    total = lib.cluster_layout(ctypes.c_uint64(n), int(diag), at, alias)
    assert total != 2**64 - 1, "bytes() is not the layout's end"
    at = dict(zip(CLUSTER, at))
    align = lib.region_align()
    assert align == 16 and lib.block() == 256
    _check_regions(at, _cluster_needs(n, diag), total, align)
    for (name, owner), got in zip(CLUSTER_ALIASES.items(), alias):
        assert got == at[owner], "%s is declared an alias of %s" % (name, owner)
    if not diag:
        assert at["pk_diag"] == total, "no diagnostic records, no room for them"
    assert total <= _parent_cluster_bytes(n, diag) + 1024
    assert total <= lib.scan_offset(ctypes.c_uint64(total)) < total + 256 and lib.scan_offset(ctypes.c_uint64(total)) % 256 == 0


@pytest.mark.parametrize("n", SIZES)
def test_probe_layout(lib, n):
    at = (ctypes.c_uint64 * len(PROBE))()
    total = lib.probe_layout(ctypes.c_uint64(n), at)
    assert total != 2**64 - 1, "bytes() is not the layout's end"
    _check_regions(dict(zip(PROBE, at)), _probe_needs(n), total, lib.region_align())
    assert total < _parent_probe_bytes(n)
