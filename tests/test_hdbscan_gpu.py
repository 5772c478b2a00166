"""TrueKNN.linkage, hdbscan_labels and hdbscan (tknnLinkage, tknnHdbscanLabels, tknnHdbscan) against tests/hdbscan_spec.py.  Every
integer array and the lambdas are compared exactly; the stabilities, whose order of addition is not fixed, within 1e-9 relative
(n * 2^-53 is 5e-13 at n = 4096), and the sets are those whose excess-of-mass decisions have a margin >= 1e-6
(tests/test_hdbscan_expectations.py), so the labels do not depend on that order.

| case          | input                                                        | catches                                                    |
|---------------|--------------------------------------------------------------|------------------------------------------------------------|
| trees         | path, star, caterpillar, random tree of 3 000, random ranks  | groups, thresholds, the chains' sizes and parents          |
| long chains   | a path whose ranks rise / fall along it                      | one chain of 2 999 pointers: the jump passes               |
| tiny          | n = 1, 2, 3, 16, 17, 63, 64, 65                              | no record, one record, wave and block borders              |
| forest        | a tree less 5 records, and a vertex in no record             | several roots                                              |
| max_rounds 1  | path and random tree                                         | the host's union-find over supervertices                   |
| lattice       | tknnEmst's records of the 12^3 lattice: all weights equal    | order by names only; scipy's Z                             |
| sets          | uniform, mixture, planar, duplicates, nan, far x mcs x ms    | the condensed tree, stabilities, selection, numbering      |
| ids           | duplicates built with permuted ids                           | names mapped back to rows                                  |
| edges         | min_cluster_size > n, n = 1                                  | all noise                                                  |
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import emst_spec as em  # noqa: E402
import hdbscan_spec as hs  # noqa: E402

pytestmark = pytest.mark.gpu

TREE = ("parent", "left", "right", "size")


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def bare():
    """An engine without a tree: tknnLinkage and tknnHdbscanLabels need none."""
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    yield eng
    eng.close()


def _engine(P, ids=None):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(np.array(P), ids=None if ids is None else np.array(ids))
    return eng


def _same_tree(got, want, what):
    for name in TREE:
        assert np.array_equal(_np(got[name]), want[name]), (what, name)


def _linkage(bare, n, u, v, what, max_rounds=0):
    got = bare.linkage(u, v, n=n, max_rounds=max_rounds)
    _same_tree(got, hs.dendrogram(n, u, v), what)
    info = got["info"]
    assert info["roots"] == n - len(u) and info["absorbed"] + info["host_edges"] == len(u) and info["rounds"] <= 64, (what, info)
    return info


@pytest.mark.parametrize("kind", ("path", "star", "caterpillar", "random"))
def test_linkage_of_trees(bare, kind):
    n = 3000
    u, v = hs.tree(kind, n, seed=7)
    info = _linkage(bare, n, u, v, kind)
    assert info["host_edges"] == 0 and 1 <= info["rounds"] <= 12 and info["solve_ms"] > 0, info


@pytest.mark.parametrize("ranks", ("along", "against"))
def test_linkage_of_one_long_chain(bare, ranks):
    """Every vertex of the path points at its neighbour: one group, one chain of n - 1 pointers and of n - 1 merges."""
    n = 3000
    u, v = hs.tree("path", n, ranks="along")
    if ranks == "against":
        u, v = (n - 1 - v).astype(np.int32), (n - 1 - u).astype(np.int32)
    info = _linkage(bare, n, u, v, ranks)
    assert info["rounds"] == 1 and info["host_edges"] == 0


@pytest.mark.parametrize("n", em.TINY_N)
def test_linkage_tiny(bare, n):
    u, v = hs.tree("random", n, seed=n) if n > 1 else (np.zeros(0, np.int32), np.zeros(0, np.int32))
    _linkage(bare, n, u, v, n)


def test_linkage_of_a_forest(bare):
    n = 3000
    u, v = hs.tree("random", n, seed=11)
    keep = np.ones(n - 1, bool)
    keep[[0, 17, 1500, 2990, 2998]] = False
    info = _linkage(bare, n + 1, u[keep], v[keep], "forest")  # (vertex n is in no record)
    assert info["roots"] == 7
    got = bare.linkage(u[keep], v[keep], n=n + 1)
    assert _np(got["parent"])[n] == -1


@pytest.mark.parametrize("kind", ("path", "random"))
def test_linkage_finished_on_the_host(bare, kind):
    n = 3000
    u, v = hs.tree(kind, n, seed=7)
    info = _linkage(bare, n, u, v, kind, max_rounds=1)
    assert info["rounds"] == 1 and info["host_edges"] > 0 and info["host_edges"] == hs.contraction(n, u, v, max_rounds=1)["host_edges"]


def test_linkage_with_all_weights_equal(bare):
    """The lattice: tknnEmst orders its records by names alone; with its weights the result is a linkage matrix."""
    from owlraytracing_amd.trueknn import linkage, linkage_matrix

    P, _, _, tree = em.case("lattice")
    n = len(P)
    assert (tree["w"] == tree["w"][0]).all()
    got = bare.linkage(np.array(tree["u"]), np.array(tree["v"]), np.array(tree["w"]), n=n)
    want = hs.dendrogram(n, tree["u"], tree["v"])
    _same_tree(got, want, "lattice")
    Z = linkage_matrix(got)
    assert Z.dtype == np.float64 and np.array_equal(Z, hs.linkage_matrix(want, tree["w"]))
    one = linkage(np.array(tree["u"]), np.array(tree["v"]), np.array(tree["w"]))
    assert np.array_equal(linkage_matrix(one), Z) and one["info"]["roots"] == 1


def _check_labels(got, want, n, what, tol=1e-9):
    info = got["info"]
    assert np.array_equal(_np(got["labels"]), want["labels"]), what
    assert (info["clusters"], info["noise"], info["condensed_clusters"]) == (want["clusters"], want["noise"], want["condensed_clusters"]), (what, info)
    assert np.array_equal(_np(got["lam"]).view(np.uint64), want["lam"].view(np.uint64)), (what, "lambda is one fp64 division")
    _same_tree(got, want["dendrogram"], what)
    stab = _np(got["stability"])
    heads = np.array(sorted(want["stability"]), np.int64)
    ref = np.array([want["stability"][h] for h in heads.tolist()])
    assert np.array_equal(np.flatnonzero(stab), heads[ref > 0] - n), what
    worst = float(np.max(np.abs(stab[heads - n] - ref) / np.maximum(ref, np.finfo(np.float64).tiny), initial=0.0))
    print("%s: stabilities off by at most %.3g relative, margin %.3g" % (what, worst, want["margin"]))
    assert worst <= tol, (what, worst)
    assert info["host_edges"] == 0 and info["solve_ms"] > 0


@pytest.mark.parametrize("name,min_samples", hs.GPU_CASES)
def test_hdbscan_of_sets(name, min_samples):
    P = hs.points(name)
    n = len(P)
    eng = _engine(P)
    before = eng.knn(k=3)
    for mcs in hs.MIN_CLUSTER_SIZES:
        what = (name, min_samples, mcs)
        want = hs.hdbscan_case(name, mcs, min_samples)
        got = eng.hdbscan(mcs, min_samples, want_tree=True, want_linkage=True, want_lambda=True, want_core_dist=True, want_stability=True)
        tree = want["tree"]
        assert (got["edges"], got["info"]["edges"], got["info"]["excluded"]) == (tree["edges"], tree["edges"], tree["excluded"]), what
        _check_labels(got, want, n, what)
        # the records are tknnEmst's on the same engine, the core distances tknnKnn's
        core = eng.knn(k=min_samples - 1)["dist"][:, -1].contiguous() if min_samples > 1 else None
        rec = eng.emst(core_dist=core)
        for f in ("u", "v", "w"):
            assert np.array_equal(_np(got[f]).view(np.int32), _np(rec[f]).view(np.int32)), (what, f)
        assert np.array_equal(_np(got["w"]).view(np.uint32), tree["w"].view(np.uint32)), what
        if core is not None:
            assert np.array_equal(_np(got["core_dist"]).view(np.uint32), _np(core).view(np.uint32)), what
        else:
            assert "core_dist" not in got
        # the same labels from the records alone
        alone = eng.hdbscan_labels(rec["u"], rec["v"], rec["w"], n, mcs, want_linkage=True, want_lambda=True, want_stability=True)
        _check_labels(alone, want, n, what + ("labels",))
        # the defaults: min_samples = min_cluster_size, nothing but labels
        if mcs == min_samples - 1:
            plain = eng.hdbscan(min_cluster_size=min_samples)
            assert set(plain) == {"labels", "edges", "info"} and np.array_equal(_np(plain["labels"]), hs.hdbscan_case(name, min_samples, min_samples)["labels"])
    after = eng.knn(k=3)
    assert all(np.array_equal(_np(before[f]).view(np.int32), _np(after[f]).view(np.int32)) for f in ("idx", "dist", "counts")), "the tree is only read"
    eng.close()


def test_hdbscan_on_a_tree_built_with_ids():
    from owlraytracing_amd.trueknn import hdbscan

    P = hs.points("duplicates")
    n = len(P)
    ids = em.permuted_ids(n, True)
    eng = _engine(P, ids)
    for mcs, ms in ((5, 1), (5, 6)):
        want = hs.hdbscan_case("duplicates", mcs, ms, ids=ids)
        got = eng.hdbscan(mcs, ms, want_tree=True, want_linkage=True, want_lambda=True, want_stability=True)
        assert np.array_equal(_np(got["u"]), want["tree"]["u"]) and np.array_equal(_np(got["v"]), want["tree"]["v"]), "the records name ids"
        _check_labels(got, want, n, ("ids", mcs, ms))
    eng.close()
    one = hdbscan(P, 5, 6)
    assert np.array_equal(one["labels"], hs.hdbscan_case("duplicates", 5, 6)["labels"]) and one["labels"].dtype == np.int32


def test_all_noise():
    P = hs.points("planar")[:300]
    eng = _engine(P)
    got = eng.hdbscan(301, 1, want_lambda=True, want_linkage=True)
    assert (_np(got["labels"]) == -1).all() and (_np(got["lam"]) == 0).all()
    assert (got["info"]["clusters"], got["info"]["noise"], got["info"]["condensed_clusters"], got["edges"]) == (0, 300, 0, 299)
    got = eng.hdbscan(300, 1)  # the whole set is one root cluster, which never wins
    assert (_np(got["labels"]) == -1).all() and got["info"]["condensed_clusters"] == 1 and got["info"]["clusters"] == 0
    eng.build(P[:1])
    for ms in (1, 3):
        got = eng.hdbscan(2, ms, want_tree=True, want_linkage=True, want_lambda=True)
        assert _np(got["labels"]).tolist() == [-1] and _np(got["parent"]).tolist() == [-1] and got["edges"] == 0 and len(got["u"]) == 0
        assert got["info"]["noise"] == 1 and got["info"]["excluded"] == (1 if ms > 1 else 0)
    eng.close()
