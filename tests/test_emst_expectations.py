"""What the GPU tests of tknnEmst expect (tests/emst_spec.py), checked on the CPU: the spec's weights against scipy's minimum
spanning tree, that the cases can catch what they are meant to catch, and that the header include/owlknn_emst.h, the ctypes
records of owlraytracing_amd/_emst_lib.py and the library agree.  Runs without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import emst_spec as em  # noqa: E402

ARG = -1


def _scipy_weights(W):
    """The sorted weights of scipy's minimum spanning forest of the dense matrix W (+inf: no edge; scipy drops zero entries, so
    only for sets without zero weights)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree

    finite = np.isfinite(W)
    assert (W[finite] > 0).all()
    T = minimum_spanning_tree(csr_matrix(np.where(finite, W, 0).astype(np.float64)))  # (float64 holds every float32 exactly)
    return np.sort(T.data.astype(np.float32))


@pytest.mark.parametrize("name", em.NO_ZERO_WEIGHTS)
def test_the_spec_has_scipys_weights(name):
    """The multiset of a minimum spanning forest's weights is unique, whatever the ties: the equality is exact."""
    P, core, _, want = em.case(name)
    W, ok = em.weights(P, core)
    assert np.array_equal(np.sort(want["w"]), _scipy_weights(W)), name
    assert want["edges"] + want["components"] == ok.sum() and want["excluded"] == len(P) - ok.sum()
    # the records: u < v, ascending by the strict key, the weights those of the matrix
    key = (want["w"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | want["u"].astype(np.uint64)
    assert (want["u"] < want["v"]).all() and (np.diff(key.astype(np.int64)) >= 0).all()
    assert np.array_equal(W[want["u"], want["v"]].view(np.uint32), want["w"].view(np.uint32))
    # the components of the records are the spec's, named by their smallest row
    lab = em.labels_of_edges(len(P), want["u"], want["v"])
    assert np.array_equal(np.where(ok, lab, -1), want["component"]) and len(np.unique(lab[ok])) == want["components"]


def test_the_cases_have_what_they_are_for():
    far = em.case("far")[3]
    assert far["components"] == 2 and far["edges"] == 598 and far["excluded"] == 0
    nan = em.case("nan")[3]
    assert nan["excluded"] == 23 and nan["components"] == 1 and (nan["component"] == -1).sum() == 23
    dup = em.case("duplicates")[3]
    assert (dup["w"] == 0).sum() == 69, "70 copies of one point are joined by 69 edges of weight 0"
    same = em.case("identical")[3]
    assert same["edges"] == 99 and (same["w"] == 0).all() and (same["u"] == 0).all(), "all keys decided by names: a star around row 0"
    bad = em.case("mutual_bad_cores")[3]
    assert bad["excluded"] == 3 and (bad["component"][[5, 77, 130]] == -1).all() and bad["component"][200] >= 0
    for n in em.TINY_N:
        t = em.case("tiny%d" % n)[3]
        assert t["edges"] == n - 1 and t["components"] == 1
    assert em.round_bound(1) == 1 and em.round_bound(2) == 2 and em.round_bound(1000) == 11 and em.round_bound(4096) == 13


def test_the_tied_cases_can_catch_a_wrong_tie_rule():
    """Tied weights among the tree's edges, and ids that reverse the order of the rows: a rule that is not the key's gives
    other records."""
    lat = em.case("lattice")[3]
    assert (lat["w"] == np.float32(1 / 32)).all() and lat["edges"] == 12 ** 3 - 1, "every edge of the lattice's tree is tied"
    mut = em.case("mutual_uniform")[3]
    bits = mut["w"].view(np.uint32)
    assert (bits[1:] == bits[:-1]).sum() >= 20, "mutual reachability: weights repeat (a core distance serves several edges)"
    by_row = em.case("duplicates")[3]
    for name in ("ids_below_n", "ids_above_n"):
        _, _, ids, by_id = em.case(name)
        assert np.array_equal(np.sort(by_id["w"]), np.sort(by_row["w"]))
        inv = {int(i): r for r, i in enumerate(ids)}
        rows = {(min(inv[a], inv[b]), max(inv[a], inv[b])) for a, b in zip(by_id["u"].tolist(), by_id["v"].tolist())}
        assert rows != set(zip(by_row["u"].tolist(), by_row["v"].tolist())), "the ids pick other edges among the tied ones"


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"TKNN_API[^;(]*?\b(tknn\w+)\s*\(", text))


def test_header_binding_and_struct_layouts_agree(tmp_path):
    """tknnEmst is declared in its own header, exported and bound with its signature, nothing was added to the other headers or
    tables, and the ctypes records have the header's sizes and offsets (gcc, C99)."""
    from owlraytracing_amd import _batch_lib, _emst_lib, _knn_lib, _lib, _periodic_lib

    assert _declared("owlknn_emst.h") == set(_emst_lib.SIGNATURES) == {"tknnEmst"}
    for header, table in (("owlknn.h", _lib), ("owlknn_knn.h", _knn_lib), ("owlknn_periodic.h", _periodic_lib), ("owlknn_batch.h", _batch_lib)):
        assert "tknnEmst" not in _declared(header) and "tknnEmst" not in table.SIGNATURES and not hasattr(table, "EmstOptions")
    res, args = _emst_lib.SIGNATURES["tknnEmst"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.POINTER(_emst_lib.EmstOptions), ctypes.POINTER(_emst_lib.EmstInfo), ctypes.c_void_p]
    pairs = {"tknnEmstOptions": _emst_lib.EmstOptions, "tknnEmstInfo": _emst_lib.EmstInfo}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn_emst.h"', "int main(void) {"]
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
    assert ctypes.sizeof(_emst_lib.EmstOptions) == 48 and ctypes.sizeof(_emst_lib.EmstInfo) == 72
    lib = _emst_lib.load()
    assert lib is _lib.load() and lib.tknnEmst.restype is ctypes.c_int and lib.tknnEmst.argtypes == args
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT tknnEmst$", exported, flags=re.M), "the library exports the symbol"
    for name in ("emst.hip", "owlknn_emst.h"):
        assert all(name in v for v in _lib._NOT_IN.values()), "the per-kernel profile records of team_* and db_* do not depend on it"


def test_a_null_engine_is_refused_without_a_device():
    from owlraytracing_amd import _emst_lib

    lib = _emst_lib.load()
    o, info = _emst_lib.EmstOptions(), _emst_lib.EmstInfo()
    info.edges = 99
    assert lib.tknnEmst(None, ctypes.byref(o), ctypes.byref(info), None) == ARG
    text = lib.tknnLastError().decode()
    assert text.startswith("tknnEmst") and "engine" in text and info.edges == 99, text
