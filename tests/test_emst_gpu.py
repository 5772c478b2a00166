"""TrueKNN.emst (tknnEmst) against tests/emst_spec.py: u, v, the bits of w, edges, components and the rows' components are
compared exactly, no tolerances.

| case        | set                                                      | catches                                                          |
|-------------|----------------------------------------------------------|------------------------------------------------------------------|
| sets        | uniform 2 048, 3-component mixture 3 000, planar, a line | the walk, pruning, late rounds with few components               |
| lattice     | 12^3, spacing 1/32                                       | every nearest distance tied: cycles or lost edges                |
| duplicates  | 70 copies of one point among 1 000; 100 identical points | zero weights, a bound of 0, all keys decided by names            |
| tiny        | n = 1, 2, 3, 16, 17, 63, 64, 65                          | a tree without internal nodes, block borders                     |
| nan / far   | 23 NaN points among 700; two clusters at x = +-3e38      | excluded points, a forest of two trees, the filled tail          |
| ids         | the duplicates set, permuted ids < n and ids >= n        | names and the tie order by id                                    |
| mutual      | uniform and duplicates, core = 5th column of knn         | weights dominated by core distances; cores that exclude points   |
| morton      | uniform, tree built under TKNN_CURVE=morton              | no dependence on the curve                                       |
| other calls | uniform 4 096                                            | dbscan(min_pts = 1), knn(k = 1), the round bound, repeats, solve |
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import emst_spec as em  # noqa: E402

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _engine(P, ids=None):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(np.array(P), ids=None if ids is None else np.array(ids))
    return eng


def _same(got, want, n, what):
    """Every output word of the call against the spec's, the filled tail included (through the library's own buffers)."""
    info = got["info"]
    assert (got["edges"], info["edges"], info["components"], info["excluded"]) == (want["edges"], want["edges"], want["components"], want["excluded"]), what
    assert np.array_equal(_np(got["u"]), want["u"]) and np.array_equal(_np(got["v"]), want["v"]), what
    assert np.array_equal(_np(got["w"]).view(np.uint32), want["w"].view(np.uint32)), what
    assert np.array_equal(_np(got["components"]), want["component"]), what
    assert 0 <= info["rounds"] <= em.round_bound(n), (what, info["rounds"])
    for name in ("u", "v", "w"):  # the slices are views of the n - 1 rows the library wrote: the tail is behind them
        full = got[name]._base if got[name]._base is not None else got[name]
        tail = _np(full)[want["edges"]:]
        assert len(full) == max(n - 1, 0) and (np.isposinf(tail).all() if name == "w" else (tail == -1).all()), (what, name)


def _check(name, eng=None):
    P, core, ids, want = em.case(name)
    own = eng is None
    eng = _engine(P, ids) if own else eng
    got = eng.emst(core_dist=core, want_components=True)
    _same(got, want, len(P), name)
    if own:
        eng.close()
    return got


@pytest.mark.parametrize("name", em.SET_NAMES)
def test_sets(name):
    got = _check(name)
    info = got["info"]
    assert info["node_tests"] > 0 and info["point_tests"] > 0 and info["rounds"] >= 2
    assert info["skipped_subtrees"] > 0, "later rounds step over subtrees of the walking point's own component"
    assert info["solve_ms"] >= info["walk_ms"] > 0 and info["merge_ms"] > 0 and info["sort_ms"] > 0


def test_lattice():
    _check("lattice")


@pytest.mark.parametrize("name", ("duplicates", "identical"))
def test_duplicates(name):
    _check(name)


@pytest.mark.parametrize("n", em.TINY_N)
def test_tiny(n):
    got = _check("tiny%d" % n)
    assert got["edges"] == n - 1 and got["info"]["components"] == 1


@pytest.mark.parametrize("name", ("nan", "far"))
def test_excluded_points_and_forests(name):
    got = _check(name)
    assert got["info"]["components"] == (2 if name == "far" else 1) and got["info"]["excluded"] == (23 if name == "nan" else 0)


@pytest.mark.parametrize("name", ("ids_below_n", "ids_above_n"))
def test_ids(name):
    _check(name)


@pytest.mark.parametrize("name", ("mutual_uniform", "mutual_duplicates", "mutual_bad_cores"))
def test_mutual_reachability(name):
    """The core distances are the 5th column of the engine's own kNN rows (bit for bit the spec's), on the device."""
    P, core, _, want = em.case(name)
    eng = _engine(P)
    col = eng.knn(k=em.MIN_SAMPLES - 1)["dist"][:, -1].contiguous()
    if name == "mutual_bad_cores":
        assert np.array_equal(em.bad_core(_np(col)).view(np.uint32), core.view(np.uint32))
        col = core
    else:
        assert np.array_equal(_np(col).view(np.uint32), core.view(np.uint32))
    _same(eng.emst(core_dist=col, want_components=True), want, len(P), name)
    if name == "mutual_uniform":
        from owlraytracing_amd.trueknn import mutual_reachability_mst

        one = mutual_reachability_mst(P, em.MIN_SAMPLES)
        assert np.array_equal(one["u"], want["u"]) and np.array_equal(one["v"], want["v"]) and np.array_equal(one["w"].view(np.uint32), want["w"].view(np.uint32))
        plain = mutual_reachability_mst(P, 1)
        assert np.array_equal(plain["w"].view(np.uint32), em.case("uniform")[3]["w"].view(np.uint32)) and "core_dist" not in plain
    eng.close()


def test_a_morton_tree(monkeypatch):
    monkeypatch.setenv("TKNN_CURVE", "morton")
    eng = _engine(em.case("uniform")[0])
    assert eng.export_tree_ex()["curve"] == 1
    _check("uniform", eng)
    eng.close()


def test_agrees_with_the_other_calls():
    import torch

    from owlraytracing_amd import datasets
    from owlraytracing_amd.trueknn import emst

    P, _, _, want = em.case("uniform4096")
    n = len(P)
    eng = _engine(P)
    r0 = datasets.start_radius(n, 5)
    before = eng.solve(5, r0)
    got = eng.emst(want_components=True)
    _same(got, want, n, "uniform4096")
    assert got["info"]["rounds"] <= em.round_bound(n) == 13
    # single linkage: the tree cut at eps is DBSCAN with min_pts = 1
    u, v, w = _np(got["u"]), _np(got["v"]), _np(got["w"])
    for eps in np.float32([0.02, 0.035, 0.05]):
        labels = _np(eng.dbscan(float(eps), 1)["labels"])
        cut = em.labels_of_edges(n, u[w <= eps], v[w <= eps])
        assert len(np.unique(labels)) == len(np.unique(cut)) > 1, eps
        pairs = np.unique(np.stack([labels, cut], axis=1), axis=0)
        assert len(pairs) == len(np.unique(cut)), "the two partitions are one"
    # the cut property: every point's nearest neighbour edge is in the tree, and the tie orders agree
    nn = eng.knn(k=1)
    a, b = np.arange(n), _np(nn["idx"])[:, 0]
    edges = set(zip(u.tolist(), v.tolist()))
    assert all((min(i, j), max(i, j)) in edges for i, j in zip(a.tolist(), b.tolist()))
    # twice: the same bits; the state of the solve is untouched
    again = eng.emst(want_components=True)
    for name in ("u", "v", "w", "components"):
        assert torch.equal(got[name].view(torch.int32), again[name].view(torch.int32)), name
    after = eng.solve(5, r0)
    for name in ("idx", "dist", "intersections"):
        assert torch.equal(before[name], after[name]), name
    eng.close()
    one = emst(P)
    assert np.array_equal(one["u"], want["u"]) and np.array_equal(one["v"], want["v"]) and one["edges"] == n - 1


def test_the_round_guard():
    """max_rounds below what the set needs: TKNN_E_ROUNDS; a max_rounds above the bound is cut to it."""
    from owlraytracing_amd._lib import TknnError

    P, _, _, want = em.case("uniform")
    eng = _engine(P)
    with pytest.raises(TknnError) as err:
        eng.emst(max_rounds=1)
    assert err.value.code == -4 and "tknnEmst" in str(err.value)
    _same(eng.emst(want_components=True, max_rounds=1000), want, len(P), "a large max_rounds")
    eng.close()
