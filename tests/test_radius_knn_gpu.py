"""TrueKNN.radius_knn (tknnRadiusKnn: at most k nearest points of the built set within a radius of points that are not in it,
as dense rows) against tests/radius_knn_spec.py on a GPU: idx, dist and counts of every row, bit for bit.  n <= 4 096 and
m <= 600 throughout.

| case        | P                                  | Q, r, k                                                                          |
|-------------|------------------------------------|----------------------------------------------------------------------------------|
| sets        | the sets of radius_spec, cut       | r0 x 1 and x 3 at the k of radius_knn_spec.SET_CASES (rows shorter and longer)   |
| dense       | 4 096 uniform                      | 256 queries in and around the cube, r = 0.2, every k of K_ALL (every list size)  |
| lattice     | spacing 1/32                       | r = 1/32 exactly, the float below, sqrt(3)/64; k = 1, 3, 6, 7 (cuts inside ties) |
| chunks      | 4 096 uniform                      | rows of 0, 1, 15, 16, 17, 63, 64, 65 entries against k = 16, 17, 64              |
| in reach    | 4 096 uniform                      | r = 4: the exact k nearest; the gate prunes                                      |
| fallback    | sets, dense, lattice               | TKNN_RADIUS_KNN_FORCE_FALLBACK=1: the one-query-per-lane kernel, identical rows  |
"""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import dbscan_query_spec as ds  # noqa: E402
import query_spec as qs  # noqa: E402
import radius_knn_spec as ks  # noqa: E402
import radius_spec as rs  # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = -1, -3, -5


def _engine(P, ids=None):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(P, ids=ids)
    return eng


def _np(v):
    return np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v)


def _same(got, want, what):
    """The engine's dense rows (tensors or arrays) equal the spec's: counts, indices, the distances' bits, the padding."""
    idx, dist, counts = _np(got["idx"]), _np(got["dist"]), _np(got["counts"])
    assert idx.dtype == np.int32 and dist.dtype == np.float32 and counts.dtype == np.int32
    assert idx.shape == want["idx"].shape and dist.shape == want["dist"].shape and counts.shape == want["counts"].shape, what
    bad = np.flatnonzero(counts != want["counts"])
    assert not len(bad), "%s: %d of %d counts differ (first: row %d, %d for %d)" % (what, len(bad), len(counts), bad[0], counts[bad[0]], want["counts"][bad[0]])
    bad = np.flatnonzero((dist.view(np.int32) != want["dist"].view(np.int32)).any(axis=1))
    assert not len(bad), "%s: %d of %d rows differ in their distances (first: row %d)" % (what, len(bad), len(dist), bad[0])
    bad = np.flatnonzero((idx != want["idx"]).any(axis=1))
    assert not len(bad), "%s: %d of %d rows differ in their indices (first: row %d, %s for %s)" % (what, len(bad), len(idx), bad[0], idx[bad[0]], want["idx"][bad[0]])
    if "info" in got and "lengths" in want:
        assert got["info"]["total"] == want["counts"].sum() and got["info"]["full_rows"] == (want["counts"] == idx.shape[1]).sum(), what


def _by_set(cases):
    """[(name, factor, (k, ..))]: one engine and one build per set and radius"""
    groups = {}
    for name, factor, k in cases:
        groups.setdefault((name, factor), []).append(k)
    return [(name, factor, tuple(kk)) for (name, factor), kk in groups.items()]


# ---- 1. sets -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,factor,kk", _by_set(ks.SET_CASES), ids=lambda v: str(v).replace(" ", ""))
def test_rows_equal_the_spec(name, factor, kk):
    P, Q, r, rows = ks.set_rows(name, factor)
    eng = _engine(P)
    for k in kk:
        got = eng.radius_knn(Q, k, radius=r)
        _same(got, ks.cut_rows(rows, k), "%s x%d k=%d" % (name, factor, k))
        assert got["info"]["lane_rows"] == 0 and got["info"]["point_tests"] >= got["info"]["total"]
    eng.close()


@pytest.mark.parametrize("k", ks.K_ALL)
def test_dense_rows_at_every_list_size(k):
    P, Q, r, rows = ks.dense_rows()
    eng = _engine(P)
    _same(eng.radius_knn(Q, k, radius=r), ks.cut_rows(rows, k), "dense k=%d" % k)
    eng.close()


# ---- 2. lattice ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 1, 2])
def test_lattice_ties_and_boundary(t):
    """r = 1/32 exactly: the six neighbours at distance exactly r are in, k = 3 cuts inside the tie and the index decides; the float
    below: they are out."""
    P, Q, radii = rs.lattice_case()
    rows = rs.rows_of(("lattice", t), lambda: rs.radius_rows(P, Q, radii[t]))
    eng = _engine(P)
    for k in ks.LATTICE_K:
        want = ks.cut_rows(rows, k)
        _same(eng.radius_knn(Q, k, radius=radii[t]), want, "lattice r=%r k=%d" % (float(radii[t]), k))
        if t == 1:
            assert (want["dist"][np.isfinite(want["dist"])] < rs.LATTICE_STEP).all()
    eng.close()


# ---- 3. chunks -----------------------------------------------------------------------------------------------------------------
def test_chunk_edges():
    P, Q, picks = rs.chunk_case()
    eng = _engine(P)
    for L, j, r in picks:
        rows = rs.radius_rows(P, Q, r)
        assert rows["lengths"][j] == L
        for k in ks.CHUNK_K:
            got = eng.radius_knn(Q, k, radius=r)
            _same(got, ks.cut_rows(rows, k), "chunks L=%d k=%d" % (L, k))
            idx, dist = _np(got["idx"])[j], _np(got["dist"])[j]
            assert (idx[min(L, k):] == -1).all() and np.isposinf(dist[min(L, k):]).all() and (idx[:min(L, k)] >= 0).all(), (L, k)
    eng.close()


# ---- 4. everything in reach ----------------------------------------------------------------------------------------------------
def test_everything_in_reach_is_the_exact_knn_and_the_gate_prunes():
    P, Q = ks.uniform_case()
    k = 10
    eng = _engine(P)
    got = eng.radius_knn(Q, k, radius=4.0)
    idx, dist = qs.exact_rows(P, Q, k)
    assert np.array_equal(_np(got["idx"]), idx) and np.array_equal(_np(got["dist"]).view(np.int32), dist.view(np.int32))
    assert (_np(got["counts"]) == k).all() and got["info"]["full_rows"] == len(Q) and got["info"]["total"] == k * len(Q)
    fill = eng.radius_query(Q, 4.0)["info"]
    print("point tests: radius_knn %d, radius_query's fill pass %d, ratio %.4f" % (got["info"]["point_tests"], fill["point_tests"],
                                                                                 got["info"]["point_tests"] / fill["point_tests"]))
    assert 0 < got["info"]["point_tests"] < fill["point_tests"], "the gate shrinks as the list fills"
    eng.close()


# ---- 5. fallback ---------------------------------------------------------------------------------------------------------------
def test_forced_fallback_gives_identical_rows(monkeypatch):
    """TKNN_RADIUS_KNN_FORCE_FALLBACK=1 (read per call): the walk leaves every query to the one-query-per-lane kernel."""
    monkeypatch.setenv("TKNN_RADIUS_KNN_FORCE_FALLBACK", "1")
    for name, factor, kk in _by_set([c for c in ks.SET_CASES if c[2] in ks.FALLBACK_K]):
        P, Q, r, rows = ks.set_rows(name, factor)
        eng = _engine(P)
        for k in kk:
            got = eng.radius_knn(Q, k, radius=r)
            _same(got, ks.cut_rows(rows, k), "fallback %s x%d k=%d" % (name, factor, k))
            assert got["info"]["lane_rows"] == len(Q)
        eng.close()
    P, Q, r, rows = ks.dense_rows()
    eng = _engine(P)
    for k in ks.FALLBACK_K:
        got = eng.radius_knn(Q, k, radius=r)
        _same(got, ks.cut_rows(rows, k), "fallback dense k=%d" % k)
        assert got["info"]["lane_rows"] == len(Q)
    P, Q, radii = rs.lattice_case()
    eng.build(P)
    for t in (0, 1, 2):
        rows = rs.rows_of(("lattice", t), lambda: rs.radius_rows(P, Q, radii[t]))
        for k in ks.LATTICE_K:
            got = eng.radius_knn(Q, k, radius=radii[t])
            _same(got, ks.cut_rows(rows, k), "fallback lattice %d k=%d" % (t, k))
            assert got["info"]["lane_rows"] == len(Q)
    monkeypatch.delenv("TKNN_RADIUS_KNN_FORCE_FALLBACK")
    assert eng.radius_knn(Q, 3, radius=radii[0])["info"]["lane_rows"] == 0
    eng.close()


# ---- 6. query counts and small trees ---------------------------------------------------------------------------------------------
def test_query_count_edges():
    from owlraytracing_amd import datasets

    P = datasets.uniform3d(2000, seed=64)
    rng = np.random.default_rng(65)
    eng = _engine(P)
    for m in (1, 2, 3, 4, 5, 63, 64, 65):
        Q = rng.random((m, 3), dtype=np.float32)
        _same(eng.radius_knn(Q, 5, radius=0.11), ks.knn_rows(P, Q, 5, radius=0.11), "m=%d" % m)
    empty = eng.radius_knn(np.zeros((0, 3), np.float32), 5, radius=0.11)
    assert empty["idx"].shape == (0, 5) and empty["dist"].shape == (0, 5) and empty["counts"].shape == (0,)
    assert empty["info"]["total"] == 0 and empty["info"]["solve_ms"] == 0 and empty["info"]["node_tests"] == 0
    eng.close()


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17])
def test_small_trees(n):
    rng = np.random.default_rng(66 + n)
    P = rng.random((n, 3), dtype=np.float32)
    Q = np.concatenate([P, rng.random((20, 3), dtype=np.float32)])
    eng = _engine(P)
    for k in (1, n, n + 3, 64):  # k > n: rows are never full
        for r in (0.3, 4.0):
            got = eng.radius_knn(Q, k, radius=r)
            _same(got, ks.knn_rows(P, Q, k, radius=r), "n=%d k=%d r=%g" % (n, k, r))
            if k > n:
                assert got["info"]["full_rows"] == 0
    eng.close()


# ---- 7. per-query radii ----------------------------------------------------------------------------------------------------------
def test_per_query_radii():
    import torch

    P, Q, _, _ = ks.dense_rows()
    valid = np.float32([0.2, 0.07, 0.31])
    radii = np.tile(np.float32([0.2, np.nan, 0.07, 0.0, 0.31, -1.0, np.inf]), 37)[:len(Q)]
    eng = _engine(P)
    for k in (5, 33):
        want = ks.knn_rows(P, Q, k, radii=radii)
        got = eng.radius_knn(Q, k, radii=radii)
        _same(got, want, "radii k=%d" % k)
        _same(eng.radius_knn(Q, k, radii=torch.from_numpy(radii).cuda()), want, "radii on the device")
        bad = ~(np.isfinite(radii) & (radii > 0))
        assert bad.sum() > 100 and (_np(got["counts"])[bad] == 0).all() and (_np(got["idx"])[bad] == -1).all()
        for r in valid:  # the valid rows: the single-radius call's at their radius
            one = eng.radius_knn(Q, k, radius=r)
            sel = radii == r
            assert np.array_equal(_np(got["idx"])[sel], _np(one["idx"])[sel]) and np.array_equal(_np(got["counts"])[sel], _np(one["counts"])[sel])
            assert np.array_equal(_np(got["dist"])[sel].view(np.int32), _np(one["dist"])[sel].view(np.int32))
    for both in (dict(radius=0.1, radii=radii), dict()):
        with pytest.raises(ValueError):
            eng.radius_knn(Q, 5, **both)
    with pytest.raises(ValueError):
        eng.radius_knn(Q, 5, radii=radii[:-1])
    eng.close()


# ---- 8. skip ids -----------------------------------------------------------------------------------------------------------------
def test_skip_ids_leave_out_self_and_nothing_else():
    import torch

    P = ks.knn_set("duplicates")[0]
    r = np.float32(0.09)
    n = len(P)
    own = np.arange(0, n, 7, dtype=np.int32)  # Q = a stride of P: m <= 600
    Q = np.ascontiguousarray(P[own])
    rows = rs.radius_rows(P, Q, r)
    eng = _engine(P)
    for k in (5, 17):
        plain, skipped = eng.radius_knn(Q, k + 1, radius=r), eng.radius_knn(Q, k, radius=r, skip_ids=own)
        _same(plain, ks.cut_rows(rows, k + 1), "Q = P, nothing skipped")
        want = ks.cut_rows(rows, k, own)
        _same(skipped, want, "Q = P, self skipped")
        assert not (_np(skipped["idx"]) == own[:, None]).any(), "no row holds its own point"
        assert (want["dist"][:, 0] == 0).sum() >= 50, "a coincident other point stays, at distance 0"
        # each row: the unskipped row of k + 1 minus its own point
        pi, si = _np(plain["idx"]), _np(skipped["idx"])
        held = np.flatnonzero((pi == own[:, None]).any(axis=1))
        assert len(held) > len(Q) // 2
        for j in held:
            assert np.array_equal(pi[j][pi[j] != own[j]], si[j]), j
        _same(eng.radius_knn(Q, k, radius=r, skip_ids=np.full(len(Q), -5, np.int32)), ks.cut_rows(rows, k), "a negative skip id changes nothing")
        _same(eng.radius_knn(Q, k, radius=r, skip_ids=torch.from_numpy(own).cuda()), want, "skip ids on the device")
    eng.close()
    # a tree built with ids: the skip is by id
    perm = np.random.default_rng(67).permutation(n).astype(np.int32)
    ids = (perm * 3 + 1_000_000).astype(np.int32)
    eng = _engine(torch.from_numpy(np.array(P)).cuda(), torch.from_numpy(ids.copy()).cuda())
    rows_ids = rs.radius_rows(P, Q, r, ids=ids)
    _same(eng.radius_knn(Q, 5, radius=r, skip_ids=ids[own]), ks.cut_rows(rows_ids, 5, ids[own]), "skip by id")
    _same(eng.radius_knn(Q, 5, radius=r, skip_ids=own), ks.cut_rows(rows_ids, 5), "a row number is no id here: nothing skipped")
    eng.close()


def test_radius_graph():
    from owlraytracing_amd.trueknn import radius_graph

    P = ks.knn_set("planar")[0][:600]
    r, k = np.float32(0.05), 6
    g = radius_graph(P, k, r)
    rows = rs.radius_rows(P, P, r)
    _same(g, ks.cut_rows(rows, k, np.arange(len(P))), "radius_graph")
    assert not (g["idx"] == np.arange(len(P))[:, None]).any(), "no (i, i) entry"
    assert (g["dist"][g["idx"] >= 0] <= r).all() and g["build_info"]["n"] == len(P)
    looped = radius_graph(P, k, r, loop=True)
    _same(looped, ks.cut_rows(rows, k), "radius_graph(loop=True)")
    assert (looped["idx"][:, 0] == np.arange(len(P))).mean() > 0.9 and (looped["dist"][:, 0] == 0).all()


# ---- 9. NaN and planar -----------------------------------------------------------------------------------------------------------
def test_nan_queries_nan_points_and_planar_queries():
    c = ds.cases("nan")[0]
    nan_q = np.isnan(c["Q"]).any(axis=1)
    assert nan_q.sum() == 5
    eng = _engine(c["P"])
    for r in (c["eps"], 3.0):
        for k in (3, 20):
            want = ks.knn_rows(c["P"], c["Q"], k, radius=r)
            got = eng.radius_knn(c["Q"], k, radius=r)
            _same(got, want, "nan r=%g k=%d" % (r, k))
            assert (want["counts"][nan_q] == 0).all()
            assert not np.isin(_np(got["idx"]), np.flatnonzero(np.isnan(c["P"]).any(axis=1))).any()
    eng.close()
    P, Q, r0 = ks.knn_set("planar")
    eng = _engine(P)
    flat = np.ascontiguousarray(Q[:50, :2])  # (m, 2): z = 0
    _same(eng.radius_knn(flat, 5, radius=np.float32(r0 * 3)), ks.knn_rows(P, flat, 5, radius=np.float32(r0 * 3)), "(m, 2) queries")
    eng.close()


# ---- 10. against the other calls -------------------------------------------------------------------------------------------------
def test_agrees_with_dbscan_query_and_radius_query():
    c = ds.cases("mixture")[0]
    Q = np.ascontiguousarray(c["Q"][::8])
    eng = _engine(c["P"])
    counted = eng.dbscan_query(Q, c["eps"], c["core_label"], want_counts=True)["counts"].cpu().numpy()
    full = eng.radius_query(Q, c["eps"])  # sort = 1, computed on the GPU
    off, fidx, fdist = full["offsets"].cpu().numpy(), full["idx"].cpu().numpy(), full["dist"].cpu().numpy()
    for k in (5, 33):
        got = eng.radius_knn(Q, k, radius=c["eps"])
        idx, dist, counts = _np(got["idx"]), _np(got["dist"]), _np(got["counts"])
        assert np.array_equal(counts, np.minimum(k, counted))
        assert (counted < k).any() and (counted > k).any()
        for j in range(len(Q)):
            cj = counts[j]
            assert np.array_equal(idx[j, :cj], fidx[off[j]:off[j] + cj]) and np.array_equal(dist[j, :cj].view(np.int32), fdist[off[j]:off[j] + cj].view(np.int32)), j
    eng.close()


# ---- 11. state -------------------------------------------------------------------------------------------------------------------
def test_solve_state_and_halo_tree_are_left_alone():
    import torch

    P, Q, radii = rs.lattice_case()
    rows = rs.rows_of(("lattice", 0), lambda: rs.radius_rows(P, Q, radii[0]))
    eng = _engine(P)
    before = eng.solve(5, 0.02)
    _same(eng.radius_knn(Q, 6, radius=radii[0]), ks.cut_rows(rows, 6), "between two solves")
    after = eng.solve(5, 0.02)
    for key in ("idx", "dist", "intersections"):
        assert torch.equal(before[key], after[key]), key
    eng.set_halo(P[:50] + np.float32(0.001), np.arange(50, dtype=np.int32) + 5000)
    got = eng.radius_knn(Q, 6, radius=radii[0])
    _same(got, ks.cut_rows(rows, 6), "with a halo tree set")
    assert (_np(got["idx"]) < 5000).all()
    eng.close()


# ---- 12. errors ------------------------------------------------------------------------------------------------------------------
def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _lib
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _lib.load()
    P, Q, radii = rs.lattice_case()
    r, k, m = float(radii[0]), 6, len(Q)
    want = ks.cut_rows(rs.rows_of(("lattice", 0), lambda: rs.radius_rows(P, Q, radii[0])), k)
    eng = TrueKNN(device=0)
    dev = eng.device
    q = torch.from_numpy(np.array(Q)).to(dev)
    guard = 1024
    idx = torch.full((m * k + guard,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((m * k + guard,), -7.0, dtype=torch.float32, device=dev)
    counts = torch.full((m + guard,), -7, dtype=torch.int32, device=dev)
    some_radii = torch.full((m,), r, dtype=torch.float32, device=dev)
    info = _lib.RadiusKnnInfo()

    def call(handle=None, options=True, **kw):
        o = _lib.RadiusKnnOptions()
        o.d_queries, o.m, o.k, o.radius = q.data_ptr(), m, k, r
        o.d_idx, o.d_dist, o.d_counts = idx.data_ptr(), dist.data_ptr(), counts.data_ptr()
        for name, v in kw.items():
            setattr(o, name, v)
        return lib.tknnRadiusKnn(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)

    def untouched():
        return bool((idx == -7).all()) and bool((dist == -7.0).all()) and bool((counts == -7).all())

    def text():
        return lib.tknnLastError().decode()

    # 1. missing pointers, before the state
    assert call(handle=ctypes.c_void_p()) == ARG and call(options=False) == ARG
    assert call(d_idx=None) == ARG and "d_idx" in text()
    assert call(d_queries=None) == ARG and "queries" in text()
    assert call(d_idx=None, k=0, radius=0.0) == ARG and "d_idx" in text()
    # 2. not built, before any look at the values
    assert call() == STATE and "tknnBuild" in text()
    assert call(k=0) == STATE and call(m=-1) == STATE and call(radius=0.0) == STATE and call(k=65) == STATE
    eng.build(P)
    # 3. the values
    assert call(k=0) == ARG and "k must be positive" in text()
    assert call(k=0, m=-1) == ARG and call(k=-3, radius=0.0) == ARG
    assert call(m=-1) == ARG and "2^31" in text() and call(m=2**31 - 1) == ARG
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(radius=bad) == ARG and "radius" in text()
        assert call(radius=bad, k=65) == ARG, "the radius before the k above the register lists"
    # 4. k above the register lists
    assert call(k=65) == UNSUPPORTED and "k out of range" in text()
    assert call(k=65, radius=0.0, d_radii=some_radii.data_ptr()) == UNSUPPORTED
    assert untouched(), "a refused call writes nothing"
    # m = 0: a zeroed info
    info.node_tests = 99
    assert call(m=0, d_queries=None) == 0 and info.node_tests == 0 and info.total == 0 and info.solve_ms == 0 and untouched()
    # the call itself; nothing is written behind the rows
    assert call() == 0 and info.total == want["counts"].sum() and info.full_rows == (want["counts"] == k).sum()
    assert info.solve_ms >= info.walk_ms > 0 and info.order_ms > 0 and info.node_tests > 0 and info.lane_rows == 0
    _same({"idx": idx[:m * k].view(m, k), "dist": dist[:m * k].view(m, k), "counts": counts[:m]}, want, "through ctypes")
    assert (idx[m * k:] == -7).all() and (dist[m * k:] == -7.0).all() and (counts[m:] == -7).all()
    # a radius that is not finite-positive is ignored where d_radii is given
    idx.fill_(-7), dist.fill_(-7.0), counts.fill_(-7)
    assert call(radius=float("nan"), d_radii=some_radii.data_ptr()) == 0
    _same({"idx": idx[:m * k].view(m, k), "dist": dist[:m * k].view(m, k), "counts": counts[:m]}, want, "d_radii")
    # d_dist = NULL and d_counts = NULL are accepted
    idx.fill_(-7), dist.fill_(-7.0), counts.fill_(-7)
    assert call(d_dist=None, d_counts=None) == 0 and info.total == want["counts"].sum()
    assert np.array_equal(idx[:m * k].view(m, k).cpu().numpy(), want["idx"]) and (dist == -7.0).all() and (counts == -7).all()
    eng.close()


def test_python_front_end():
    import torch

    from owlraytracing_amd.trueknn import radius_knn

    P, Q, r, rows = ks.dense_rows()
    want = ks.cut_rows(rows, 17)
    res = radius_knn(P, Q, 17, radius=r)
    _same(res, want, "one-shot helper")
    assert res["build_info"]["n"] == len(P) and isinstance(res["idx"], np.ndarray)
    eng = _engine(P)
    _same(eng.radius_knn(torch.from_numpy(np.array(Q)).cuda(), 17, radius=r), want, "a device tensor")
    only_idx = eng.radius_knn(Q, 17, radius=r, want_dist=False)
    assert "dist" not in only_idx and np.array_equal(_np(only_idx["idx"]), want["idx"])
    for bad in (Q.astype(np.float64)[:, :1], torch.from_numpy(np.array(Q)), torch.from_numpy(np.array(Q)).cuda().double(),
                torch.from_numpy(np.array(Q)).cuda()[:, :2], torch.from_numpy(np.array(Q)).cuda()[::2]):
        with pytest.raises(ValueError):
            eng.radius_knn(bad, 17, radius=r)
    eng.close()
