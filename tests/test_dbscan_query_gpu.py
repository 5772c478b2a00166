"""TrueKNN.dbscan_query (tknnDbscanQuery: cluster labels and neighbour counts for points that are not in the tree) against
tests/dbscan_query_spec.py on a GPU: every query of every set, exactly.

| set     | P                                         | Q                                                                        |
|---------|-------------------------------------------|--------------------------------------------------------------------------|
| slabs   | three slabs 1.2 eps apart, three clusters | in the gaps (two clusters in reach), around the scene, copies of P       |
| mixture | 3 000 points of a 5-component mixture     | P itself + 1 000 more of the mixture                                     |
| tiny    | n = 1, 2, 5; no core point; 64 duplicates | copies, near and far points                                              |
| nan     | 1 000 uniform, 7 with a NaN coordinate    | uniform, 5 with a NaN coordinate, copies of finite points                |
| edges   | 2 048 uniform                             | m = 1, 63, 64, 65, 255, 256, 257, some up to ten scene extents outside   |
"""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import dbscan_query_spec as ds  # noqa: E402

pytestmark = pytest.mark.gpu


def _engine(P, ids=None):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(P, ids=ids)
    return eng


def _same(r, c, what, counts=True):
    got = r["labels"].cpu().numpy()
    assert got.dtype == np.int32 and got.shape == c["labels"].shape
    bad = np.flatnonzero(got != c["labels"])
    assert not len(bad), "%s: %d of %d labels differ (first: query %d, %d for %d)" % (what, len(bad), len(got), bad[0], got[bad[0]], c["labels"][bad[0]])
    if counts:
        cnt = r["counts"].cpu().numpy()
        bad = np.flatnonzero(cnt != c["counts"])
        assert not len(bad), "%s: %d of %d counts differ (first: query %d, %d for %d)" % (what, len(bad), len(cnt), bad[0], cnt[bad[0]], c["counts"][bad[0]])
    else:
        assert "counts" not in r


@pytest.mark.parametrize("name", ds.SET_NAMES)
def test_labels_and_counts_equal_the_spec(name):
    eng = None
    for c in ds.cases(name):
        if eng is None or eng.n != len(c["P"]) or c["P"] is not last_P:
            if eng is not None:
                eng.close()
            eng, last_P = _engine(c["P"]), c["P"]
        what = "%s/%s" % (name, c["name"])
        with_counts = eng.dbscan_query(c["Q"], c["eps"], c["core_label"], want_counts=True)
        _same(with_counts, c, what)
        assert with_counts["info"]["clusters"] == -1
        without = eng.dbscan_query(c["Q"], c["eps"], c["core_label"])
        _same(without, c, what + " (no counts)", counts=False)
        assert without["info"]["point_tests"] <= with_counts["info"]["point_tests"]
    eng.close()


def test_the_set_as_queries_gives_the_clustering():
    c = ds.cases("mixture")[0]
    eng = _engine(c["P"])
    full = eng.dbscan(c["eps"], c["min_pts"], want_counts=True)
    r = eng.dbscan_query(c["P"], c["eps"], full["labels"], core=full["core"], want_counts=True)
    assert np.array_equal(r["labels"].cpu().numpy(), full["labels"].cpu().numpy())
    assert np.array_equal(r["counts"].cpu().numpy(), full["counts"].cpu().numpy())
    assert np.array_equal(full["labels"].cpu().numpy(), c["oracle"]["labels"])
    eng.close()


def test_rows_not_ids():
    import torch

    c = ds.cases("slabs")[0]
    ids = (np.random.default_rng(5).permutation(len(c["P"])).astype(np.int32) * 3 + 1_000_000).copy()
    eng = _engine(torch.from_numpy(np.array(c["P"])).cuda(), torch.from_numpy(ids).cuda())
    _same(eng.dbscan_query(c["Q"], c["eps"], c["core_label"], want_counts=True), c, "tree built with ids")
    eng.close()


def test_results_follow_the_callers_order():
    c = ds.cases("slabs")[0]
    eng = _engine(c["P"])
    perm = np.random.default_rng(6).permutation(len(c["Q"]))
    shuffled = {"labels": c["labels"][perm], "counts": c["counts"][perm]}
    _same(eng.dbscan_query(np.ascontiguousarray(c["Q"][perm]), c["eps"], c["core_label"], want_counts=True), shuffled, "shuffled queries")
    eng.close()


def test_solve_and_query_state_is_left_alone():
    """tknnSolve and tknnQuery before and after a dbscan query on the same engine return what they returned before."""
    c = ds.cases("mixture")[0]
    eng = _engine(c["P"])
    k, r0 = 5, 0.01
    Q = c["Q"][-1000:]

    def snapshot():
        s, q = eng.solve(k, r0), eng.query(Q, k, r0, want_levels=True)
        return [s[n].cpu().numpy().copy() for n in ("idx", "dist", "intersections")] + [q[n].cpu().numpy().copy() for n in ("idx", "dist", "intersections", "levels")]

    before = snapshot()
    _same(eng.dbscan_query(c["Q"], c["eps"], c["core_label"], want_counts=True), c, "between solves")
    after = snapshot()
    for x, y in zip(before, after):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
    _same(eng.dbscan_query(c["Q"], c["eps"], c["core_label"], want_counts=True), c, "after the solves")
    eng.close()


def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _lib
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _lib.load()
    c = {x["name"]: x for x in ds.cases("tiny")}["n5_minpts2"]
    eng = TrueKNN(device=0)
    dev = eng.device
    m = len(c["Q"])
    q = torch.from_numpy(np.array(c["Q"])).to(dev)
    core_label = torch.from_numpy(np.array(c["core_label"])).to(dev)
    labels = torch.full((m,), -7, dtype=torch.int32, device=dev)
    counts = torch.full((m,), -7, dtype=torch.int32, device=dev)
    info = _lib.DbscanInfo()

    def call(handle=None, options=True, **kw):
        o = _lib.DbscanQueryOptions()
        o.d_queries, o.m, o.eps = q.data_ptr(), m, c["eps"]
        o.d_core_label, o.d_labels, o.d_counts = core_label.data_ptr(), labels.data_ptr(), counts.data_ptr()
        for name, v in kw.items():
            setattr(o, name, v)
        return lib.tknnDbscanQuery(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)

    ARG, STATE = -1, -3
    assert call(handle=ctypes.c_void_p()) == ARG and call(options=False) == ARG
    assert call(d_core_label=None) == ARG and call(d_labels=None) == ARG and call(d_queries=None) == ARG
    assert call() == STATE and call(eps=0.0) == STATE and call(m=-1) == STATE  # not built: before any look at the values
    assert call(d_labels=None, eps=0.0) == ARG  # a missing pointer: before the state
    eng.build(c["P"])
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(eps=bad) == ARG
    assert call(m=-1) == ARG and call(m=2**31 - 1) == ARG
    assert (labels == -7).all() and (counts == -7).all(), "a refused call writes nothing"
    info.node_tests = 99
    assert call(m=0, d_queries=None) == 0 and info.node_tests == 0 and info.clusters == 0 and info.solve_ms == 0
    assert (labels == -7).all()
    assert call(d_counts=None) == 0 and (counts == -7).all()
    assert np.array_equal(labels.cpu().numpy(), c["labels"])
    assert call() == 0 and info.clusters == -1 and info.point_tests == info.label_point_tests and info.node_tests > 0
    assert info.solve_ms >= info.label_ms > 0
    assert np.array_equal(counts.cpu().numpy(), c["counts"])
    eng.set_halo(c["P"], np.arange(5, dtype=np.int32) + 5000)  # a halo tree is ignored
    labels.fill_(-7)
    assert call() == 0 and np.array_equal(labels.cpu().numpy(), c["labels"]) and np.array_equal(counts.cpu().numpy(), c["counts"])
    eng.close()


def test_python_front_end():
    import torch

    from owlraytracing_amd.trueknn import dbscan_query

    c = ds.cases("mixture")[0]
    r = dbscan_query(c["P"], c["Q"], c["eps"], c["min_pts"])
    assert np.array_equal(r["labels"], c["labels"]) and np.array_equal(r["counts"], c["counts"])
    assert np.array_equal(r["point_labels"], c["oracle"]["labels"]) and r["clusters"] == c["oracle"]["clusters"]
    eng = _engine(c["P"])
    empty = eng.dbscan_query(np.zeros((0, 3), np.float32), c["eps"], c["core_label"], want_counts=True)
    assert empty["labels"].shape == (0,) and empty["counts"].shape == (0,)
    planar = eng.dbscan_query(np.array(c["Q"][:10, :2]), c["eps"], c["core_label"])  # (m, 2): z = 0
    assert planar["labels"].shape == (10,)
    for bad in (c["Q"].astype(np.float64)[:, :1], torch.from_numpy(np.array(c["Q"])), torch.from_numpy(np.array(c["Q"])).cuda().double(),
                torch.from_numpy(np.array(c["Q"])).cuda()[:, :2], torch.from_numpy(np.array(c["Q"])).cuda()[::2]):
        with pytest.raises(ValueError):
            eng.dbscan_query(bad, c["eps"], c["core_label"])
    with pytest.raises(ValueError):
        eng.dbscan_query(c["Q"], c["eps"], c["core_label"][:-1])
    eng.close()
