"""What the GPU tests of tknnLinkage, tknnHdbscanLabels and tknnHdbscan expect (tests/hdbscan_spec.py), checked on the CPU: the
spec's dendrogram against scipy, its labels against sklearn's own tree code, the margin of every excess-of-mass decision on the
sets the GPU tests use, the contraction rounds of csrc/linkage.hip restated in numpy against the sequential union-find, and that
the header include/owlknn_hdbscan.h, the ctypes records of owlraytracing_amd/_hdbscan_lib.py and the library agree.  Runs without a
GPU."""
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
import hdbscan_spec as hs  # noqa: E402

ARG = -1
TREE = ("parent", "left", "right", "size")


@pytest.mark.parametrize("name", ("uniform", "planar", "blobs"))
def test_the_spec_dendrogram_is_scipys(name):
    """Single linkage of the full weight matrix: with all tree weights distinct the linkage matrix is unique, row for row."""
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform

    want = hs.hdbscan_case(name, 5, 1)
    tree, P = want["tree"], want["P"]
    assert len(P) <= 2048 and tree["edges"] == len(P) - 1
    assert len(np.unique(tree["w"])) == tree["edges"], "all tree weights distinct"
    W, _ = em.weights(P)
    Z = linkage(squareform(W.astype(np.float64), checks=False), "single")
    assert np.array_equal(Z, hs.linkage_matrix(want["dendrogram"], tree["w"]))


def _sklearn_labels(tree, min_cluster_size):
    _linkage = pytest.importorskip("sklearn.cluster._hdbscan._linkage")
    _tree = pytest.importorskip("sklearn.cluster._hdbscan._tree")
    if not (hasattr(_linkage, "make_single_linkage") and hasattr(_linkage, "MST_edge_dtype") and hasattr(_tree, "tree_to_labels")):
        pytest.skip("this sklearn keeps its HDBSCAN tree code elsewhere")
    mst = np.zeros(tree["edges"], dtype=_linkage.MST_edge_dtype)
    mst["current_node"], mst["next_node"], mst["distance"] = tree["u"], tree["v"], tree["w"]
    return _tree.tree_to_labels(_linkage.make_single_linkage(mst), min_cluster_size, "eom", False, 0.0, None)[0]


def _same_partition(a, b):
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b)) and np.array_equal(a < 0, b < 0)


@pytest.mark.parametrize("name", ("uniform", "planar", "blobs"))
@pytest.mark.parametrize("min_samples", (1, 6))
def test_the_spec_labels_are_sklearns(name, min_samples):
    """sklearn's make_single_linkage + tree_to_labels (eom, no single cluster) fed the same spanning tree: the same partition, the
    same noise.  Sets without zero weights (sklearn has an infinite lambda there)."""
    for mcs in hs.MIN_CLUSTER_SIZES:
        want = hs.hdbscan_case(name, mcs, min_samples)
        assert (want["tree"]["w"] > 0).all() and want["tree"]["edges"] == len(want["P"]) - 1
        assert _same_partition(want["labels"], _sklearn_labels(want["tree"], mcs)), (name, min_samples, mcs)
        assert want["margin"] >= 1e-6


@pytest.mark.parametrize("name,min_samples", hs.GPU_CASES)
def test_the_gpu_sets_decide_with_a_margin(name, min_samples):
    """|stability(C) - S(c1) - S(c2)| / max of the two is >= 1e-6 at every decision: the labels do not depend on the order in
    which the device adds up a stability (relative error <= n * 2^-53).  And the labels are what they say they are."""
    P = hs.points(name)
    n = len(P)
    for mcs in hs.MIN_CLUSTER_SIZES:
        want = hs.hdbscan_case(name, mcs, min_samples)
        assert want["margin"] >= 1e-6, (name, min_samples, mcs, want["margin"])
        lab = want["labels"]
        assert want["clusters"] == lab.max() + 1 and want["noise"] == (lab < 0).sum()
        first = [int(np.flatnonzero(lab == c)[0]) for c in range(want["clusters"])]
        assert first == sorted(first), "numbered by the smallest row"
        assert all((lab == c).sum() >= mcs for c in range(want["clusters"]))
        assert (want["lam"][lab >= 0] > 0).all() and all(s >= 0 for s in want["stability"].values())
        assert len(want["lam"]) == n and (lab[~em.eligible(P, want["core"])] == -1).all()
    if name == "duplicates":
        assert (hs.hdbscan_case(name, 5, 1)["lam"] == 1 / hs.FLT_MIN).sum() >= 70, "w = 0 is taken as FLT_MIN"
    if name == "far":
        assert want["tree"]["components"] == 2 and (want["dendrogram"]["parent"] == -1).sum() == 2
    if name == "nan":
        assert want["tree"]["excluded"] == 23


def test_ids_change_the_records_not_the_labels_rows():
    P = hs.points("duplicates")
    ids = em.permuted_ids(len(P), True)
    for ms in (1, 6):
        by_id, by_row = hs.hdbscan_case("duplicates", 5, ms, ids=ids), hs.hdbscan_case("duplicates", 5, ms)
        assert by_id["margin"] >= 1e-6
        assert not np.array_equal(by_id["tree"]["u"], by_row["tree"]["u"]) and by_id["tree"]["u"].min() >= 1_000_000
        assert np.array_equal(np.sort(by_id["tree"]["w"]), np.sort(by_row["tree"]["w"]))


@pytest.mark.parametrize("kind", ("path", "star", "caterpillar", "random"))
@pytest.mark.parametrize("ranks", ("random", "along"))
def test_the_contraction_rounds_equal_the_union_find(kind, ranks):
    for n in (2, 3, 16, 17, 63, 64, 65, 3000):
        u, v = hs.tree(kind, n, seed=n, ranks=ranks)
        want = hs.dendrogram(n, u, v)
        for max_rounds in (64, 1, 2):
            got = hs.contraction(n, u, v, max_rounds=max_rounds)
            assert all(np.array_equal(got[f], want[f]) for f in TREE), (kind, ranks, n, max_rounds)
            assert sum(got["absorbed"]) + got["host_edges"] == n - 1 and (got["host_edges"] == 0 or got["rounds"] == max_rounds)
        if n == 3000:
            full = hs.contraction(n, u, v)
            assert full["host_edges"] == 0 and full["rounds"] <= 12 and full["absorbed"][0] >= (n - 1) // 3
    assert (want["size"][-1], (want["parent"] == -1).sum()) == (3000, 1) and (want["left"] < want["right"]).all()


def test_the_contraction_rounds_on_spanning_trees_and_forests():
    for name, ms in (("uniform", 1), ("uniform", 6), ("far", 1), ("nan", 6)):
        want = hs.hdbscan_case(name, 5, ms)
        tree, n = want["tree"], len(want["P"])
        got = hs.contraction(n, tree["u"], tree["v"])
        assert all(np.array_equal(got[f], want["dendrogram"][f]) for f in TREE), (name, ms)
        assert got["rounds"] <= 12 and (got["parent"] == -1).sum() == n - tree["edges"]


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"TKNN_API[^;(]*?\b(tknn\w+)\s*\(", text))


def test_header_binding_and_struct_layouts_agree(tmp_path):
    from owlraytracing_amd import _batch_lib, _emst_lib, _hdbscan_lib, _knn_lib, _lib, _periodic_lib

    names = {"tknnLinkage", "tknnHdbscanLabels", "tknnHdbscan"}
    assert _declared("owlknn_hdbscan.h") == set(_hdbscan_lib.SIGNATURES) == names
    for header, table in (("owlknn.h", _lib), ("owlknn_knn.h", _knn_lib), ("owlknn_periodic.h", _periodic_lib), ("owlknn_batch.h", _batch_lib),
                          ("owlknn_emst.h", _emst_lib)):
        assert not names & _declared(header) and not names & set(table.SIGNATURES)
    pairs = {"tknnLinkageOptions": _hdbscan_lib.LinkageOptions, "tknnLinkageInfo": _hdbscan_lib.LinkageInfo,
             "tknnHdbscanLabelsOptions": _hdbscan_lib.HdbscanLabelsOptions, "tknnHdbscanLabelsInfo": _hdbscan_lib.HdbscanLabelsInfo,
             "tknnHdbscanOptions": _hdbscan_lib.HdbscanOptions, "tknnHdbscanInfo": _hdbscan_lib.HdbscanInfo}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn_hdbscan.h"', "int main(void) {"]
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
    lib = _hdbscan_lib.load()
    assert lib is _lib.load()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name, (res, args) in _hdbscan_lib.SIGNATURES.items():
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), "the library exports the symbol"
        assert getattr(lib, name).restype is res is ctypes.c_int and getattr(lib, name).argtypes == args and args[0] is args[3] is ctypes.c_void_p
    for name in ("linkage.hip", "linkage.h", "hdbscan.hip", "owlknn_hdbscan.h"):
        assert all(name in v for v in _lib._NOT_IN.values()), "the per-kernel profile records of team_* and db_* do not depend on it"
    info = _hdbscan_lib.HdbscanInfo()
    info.labels.clusters, info.edges = 3, 7
    assert info.as_dict()["clusters"] == 3 and info.as_dict()["edges"] == 7 and "labels" not in info.as_dict() and "pad_" not in info.as_dict()


@pytest.mark.parametrize("name", ("tknnLinkage", "tknnHdbscanLabels", "tknnHdbscan"))
def test_a_null_engine_is_refused_without_a_device(name):
    from owlraytracing_amd import _hdbscan_lib

    lib = _hdbscan_lib.load()
    _, args = _hdbscan_lib.SIGNATURES[name]
    o, info = args[1]._type_(), args[2]._type_()
    ctypes.memset(ctypes.byref(info), 0x5a, ctypes.sizeof(info))
    assert getattr(lib, name)(None, ctypes.byref(o), ctypes.byref(info), None) == ARG
    text = lib.tknnLastError().decode()
    assert text.startswith(name + ":") and "engine" in text, text
    assert bytes(info) == b"\x5a" * ctypes.sizeof(info), "a refused call leaves info alone"
