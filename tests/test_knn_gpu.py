"""TrueKNN.knn (tknnKnn: the k nearest points of the built set, exactly, with no radius from the caller) against tests/knn_spec.py
on a GPU: idx, dist and counts of every row, bit for bit.  n <= 4 096 and m <= 600 for external queries throughout.

| case        | P                                   | queries, k                                                                       |
|-------------|-------------------------------------|----------------------------------------------------------------------------------|
| sets        | the sets of radius_knn_spec, cut    | their queries and their own points, every k of K_ALL (every list size)           |
| lattice     | spacing 1/32                        | nodes, cell centres, edge midpoints; k = 1, 3, 6, 7: ties at the k-th place      |
| duplicates  | 1 000 uniform, 70 of them one point | that point and others; k = 1, 16, 64: a seed bound of 0                          |
| tiny        | 1, 2, 16, 17, 65 points             | k below, equal to and above the eligible count; with the skip n = k and n = k + 1|
| nan         | 700 points, 23 with a NaN           | 64 queries, 5 with a NaN                                                         |
| far         | two clusters 0.8 apart              | ten scene widths outside, first and last slot of the order, between the clusters |
| ids         | duplicates set                      | permuted ids below n, ids above n: entries, ties and skips go by id              |
| morton      | uniform                             | a tree built under TKNN_CURVE=morton                                             |
| fallback    | sets, lattice, duplicates           | TKNN_KNN_FORCE_FALLBACK=1: the one-query-per-lane kernel, identical rows         |
| other calls | uniform, duplicates                 | tknnRadiusKnn at radius 4; solve + repair_exact                                  |
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_spec as kn  # noqa: E402
import radius_knn_spec as rk  # noqa: E402

pytestmark = pytest.mark.gpu

ARG = -1


def _engine(P, ids=None):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(P, ids=ids)
    return eng


def _np(v):
    return np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v)


def _same(got, want, what):
    """The engine's dense rows (tensors or arrays) equal the spec's: counts, indices, the distances' bits, the padding; no row
    holds an index twice; the info's sums are the rows'."""
    idx, dist, counts = _np(got["idx"]), _np(got["dist"]), _np(got["counts"])
    assert idx.dtype == np.int32 and dist.dtype == np.float32 and counts.dtype == np.int32
    assert idx.shape == want["idx"].shape and dist.shape == want["dist"].shape and counts.shape == want["counts"].shape, what
    bad = np.flatnonzero(counts != want["counts"])
    assert not len(bad), "%s: %d of %d counts differ (first: row %d, %d for %d)" % (what, len(bad), len(counts), bad[0], counts[bad[0]], want["counts"][bad[0]])
    bad = np.flatnonzero((dist.view(np.int32) != want["dist"].view(np.int32)).any(axis=1))
    assert not len(bad), "%s: %d of %d rows differ in their distances (first: row %d, %s for %s)" % (what, len(bad), len(dist), bad[0], dist[bad[0]], want["dist"][bad[0]])
    bad = np.flatnonzero((idx != want["idx"]).any(axis=1))
    assert not len(bad), "%s: %d of %d rows differ in their indices (first: row %d, %s for %s)" % (what, len(bad), len(idx), bad[0], idx[bad[0]], want["idx"][bad[0]])
    if idx.shape[1] > 1:
        s = np.sort(idx, axis=1)
        assert not ((s[:, 1:] == s[:, :-1]) & (s[:, 1:] >= 0)).any(), "%s: a row holds an index twice" % what
    if "info" in got:
        info = got["info"]
        assert info["total"] == want["counts"].sum() and info["full_rows"] == (want["counts"] == idx.shape[1]).sum(), what
        assert 0 <= info["tightened_rows"] <= info["full_rows"] and info["lane_rows"] <= len(idx), what


# ---- 1. sets -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kn.SET_NAMES)
def test_external_rows_equal_the_spec(name):
    P, Q, rows = kn.set_rows(name)
    eng = _engine(P)
    for k in rk.K_ALL:
        got = eng.knn(Q, k)
        _same(got, kn.cut(rows, k), "%s k=%d" % (name, k))
        assert got["info"]["lane_rows"] == 0 and got["info"]["seed_point_tests"] >= 16 * len(Q)
    eng.close()


@pytest.mark.parametrize("name", kn.SET_NAMES)
def test_self_rows_equal_the_spec(name):
    P, rows = kn.set_self_rows(name)
    eng = _engine(P)
    for k in rk.K_ALL:
        got = eng.knn(k=k)
        _same(got, kn.cut(rows, k), "self %s k=%d" % (name, k))
        assert not (_np(got["idx"]) == np.arange(len(P))[:, None]).any(), "no row holds its own point"
        assert got["info"]["lane_rows"] == 0 and got["info"]["order_ms"] < got["info"]["solve_ms"]
    eng.close()


def test_the_walk_matters_on_the_uniform_set():
    """A kernel that only returned its seeds would have no row to tighten; every row is full, inside the cube and outside."""
    P, Q, rows = kn.set_rows("uniform")
    eng = _engine(P)
    for k in (5, 33):
        info = eng.knn(Q, k)["info"]
        assert info["tightened_rows"] > 0 and info["full_rows"] == len(Q), info
        assert info["point_tests"] > 0 and info["node_tests"] > 0 and info["solve_ms"] >= info["walk_ms"] > 0 and info["seed_ms"] > 0
        own = eng.knn(k=k)["info"]
        assert own["tightened_rows"] > 0 and own["full_rows"] == len(P), own
    eng.close()


# ---- 2. lattice, duplicates ------------------------------------------------------------------------------------------------------
def test_lattice_ties_at_the_kth_place():
    P, Q = kn.lattice_case()
    rows = kn.rows_of(("lattice",), lambda: kn.knn_rows(P, Q, max(rk.LATTICE_K)))
    own = kn.rows_of(("lattice-self",), lambda: kn.self_rows(P, max(rk.LATTICE_K)))
    eng = _engine(P)
    for k in rk.LATTICE_K:
        _same(eng.knn(Q, k), kn.cut(rows, k), "lattice k=%d" % k)
        _same(eng.knn(k=k), kn.cut(own, k), "lattice self k=%d" % k)
    eng.close()


def test_duplicates_give_a_bound_of_zero():
    P, Q = kn.duplicates_case()
    eng = _engine(P)
    for k in kn.DUPLICATE_K:
        got = eng.knn(Q, k)
        _same(got, kn.knn_rows(P, Q, k), "duplicates k=%d" % k)
        assert _np(got["dist"])[0, k - 1] == 0 and _np(got["counts"])[0] == k
        _same(eng.knn(k=k), kn.self_rows(P, k), "duplicates self k=%d" % k)
    eng.close()


# ---- 3. tiny trees -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", kn.TINY_N)
def test_tiny_trees(n):
    P, Q, ks = kn.tiny_case(n)
    eng = _engine(P)
    for k in ks:
        got = eng.knn(Q, k)
        _same(got, kn.knn_rows(P, Q, k), "n=%d k=%d" % (n, k))
        if k > n:
            assert got["info"]["full_rows"] == 0
        _same(eng.knn(k=k), kn.self_rows(P, k), "self n=%d k=%d" % (n, k))
    # with the skip: n = k (one entry short) and n = k + 1 (exactly full)
    own = np.arange(len(P), dtype=np.int32)
    for k in {min(n, kn.K_MAX), max(min(n - 1, kn.K_MAX), 1)}:
        got = eng.knn(P, k, skip_ids=own)
        _same(got, kn.knn_rows(P, P, k, skip=own), "skip n=%d k=%d" % (n, k))
        assert (_np(got["counts"]) == min(k, n - 1)).all()
    eng.close()


def test_query_count_edges():
    from owlraytracing_amd import datasets

    P = datasets.uniform3d(2000, seed=64)
    rng = np.random.default_rng(65)
    eng = _engine(P)
    for m in (1, 2, 3, 4, 5, 63, 64, 65):
        Q = rng.random((m, 3), dtype=np.float32)
        _same(eng.knn(Q, 5), kn.knn_rows(P, Q, 5), "m=%d" % m)
    empty = eng.knn(np.zeros((0, 3), np.float32), 5)
    assert empty["idx"].shape == (0, 5) and empty["dist"].shape == (0, 5) and empty["counts"].shape == (0,)
    assert empty["info"]["total"] == 0 and empty["info"]["solve_ms"] == 0 and empty["info"]["node_tests"] == 0
    eng.close()


# ---- 4. NaN, far and edge queries --------------------------------------------------------------------------------------------------
def test_nan_points_and_nan_queries():
    P, Q = kn.nan_case()
    nan_q, nan_p = np.isnan(Q).any(axis=1), np.flatnonzero(np.isnan(P).any(axis=1))
    eng = _engine(P)
    for k in (3, 20, 64):
        got = eng.knn(Q, k)
        _same(got, kn.knn_rows(P, Q, k), "nan k=%d" % k)
        assert (_np(got["counts"])[nan_q] == 0).all() and not np.isin(_np(got["idx"]), nan_p).any()
        own = eng.knn(k=k)
        _same(own, kn.self_rows(P, k), "nan self k=%d" % k)
        assert (_np(own["counts"])[nan_p] == 0).all() and not np.isin(_np(own["idx"]), nan_p).any()
    eng.close()


def test_far_queries_edge_slots_and_between_clusters():
    P, Q = kn.far_case()
    eng = _engine(P)
    order = eng.export_tree()["prim_id"]
    ends = P[[order[0], order[1], order[-2], order[-1]]]  # the first and last slots of the order, and just beside them
    Q = np.ascontiguousarray(np.concatenate([Q, ends, ends + np.float32(1e-4)]))
    for k in (1, 16, 33, 64):
        _same(eng.knn(Q, k), kn.knn_rows(P, Q, k), "far k=%d" % k)
    eng.close()


# ---- 5. ids, curve -----------------------------------------------------------------------------------------------------------------
def test_ids_name_entries_ties_and_skips():
    import torch

    P = rk.knn_set("duplicates")[0][:1500]
    n = len(P)
    rng = np.random.default_rng(77)
    own = np.arange(0, n, 3, dtype=np.int64)
    Q = np.ascontiguousarray(P[own])
    for ids in (rng.permutation(n).astype(np.int32), (rng.permutation(n) * 3 + 1_000_000).astype(np.int32)):
        eng = _engine(torch.from_numpy(np.array(P)).cuda(), torch.from_numpy(ids.copy()).cuda())
        for k in (5, 17):
            _same(eng.knn(Q, k), kn.knn_rows(P, Q, k, ids=ids), "ids k=%d" % k)
            _same(eng.knn(Q, k, skip_ids=ids[own]), kn.knn_rows(P, Q, k, skip=ids[own], ids=ids), "skip by id k=%d" % k)
            got = eng.knn(k=k)
            _same(got, kn.self_rows(P, k, ids=ids), "self by id k=%d" % k)
            assert not (_np(got["idx"]) == ids[:, None]).any()
        eng.close()


def test_a_morton_tree(monkeypatch):
    monkeypatch.setenv("TKNN_CURVE", "morton")
    P, Q, rows = kn.set_rows("uniform")
    eng = _engine(P)
    assert eng.export_tree_ex()["curve"] == 1
    for k in (5, 33):
        got = eng.knn(Q, k)
        _same(got, kn.cut(rows, k), "morton k=%d" % k)
        assert got["info"]["tightened_rows"] > 0
        _same(eng.knn(k=k), kn.cut(kn.set_self_rows("uniform")[1], k), "morton self k=%d" % k)
    eng.close()


# ---- 6. fallback -------------------------------------------------------------------------------------------------------------------
def test_forced_fallback_gives_identical_rows(monkeypatch):
    """TKNN_KNN_FORCE_FALLBACK=1 (read per call): the walk leaves every query to the one-query-per-lane kernel."""
    cases = [(name,) + kn.set_rows(name) for name in ("uniform", "duplicates", "scale_up")]
    P, Q = kn.lattice_case()
    cases.append(("lattice", P, Q, kn.rows_of(("lattice-64",), lambda: kn.knn_rows(P, Q, kn.K_MAX))))
    P, Q = kn.duplicates_case()
    cases.append(("copies of one point", P, Q, kn.rows_of(("duplicates-64",), lambda: kn.knn_rows(P, Q, kn.K_MAX))))
    for name, P, Q, rows in cases:
        eng = _engine(P)
        for k in (1, 6, 17, 64):
            plain = eng.knn(Q, k)
            own = eng.knn(k=k)
            monkeypatch.setenv("TKNN_KNN_FORCE_FALLBACK", "1")
            forced = eng.knn(Q, k)
            forced_own = eng.knn(k=k)
            monkeypatch.delenv("TKNN_KNN_FORCE_FALLBACK")
            assert plain["info"]["lane_rows"] == 0 and forced["info"]["lane_rows"] == len(Q) and forced_own["info"]["lane_rows"] == len(P)
            _same(forced, kn.cut(rows, k), "fallback %s k=%d" % (name, k))
            for a, b in ((plain, forced), (own, forced_own)):
                assert np.array_equal(_np(a["idx"]), _np(b["idx"])) and np.array_equal(_np(a["counts"]), _np(b["counts"]))
                assert np.array_equal(_np(a["dist"]).view(np.int32), _np(b["dist"]).view(np.int32))
                assert a["info"]["tightened_rows"] == b["info"]["tightened_rows"] and a["info"]["total"] == b["info"]["total"]
        eng.close()


# ---- 7. against the other calls ----------------------------------------------------------------------------------------------------
def test_agrees_with_radius_knn_at_a_radius_that_covers_the_set():
    """All of these sets lie inside the unit cube: at radius 4 tknnRadiusKnn's rows are the k nearest, with the same skips."""
    for name in ("uniform", "duplicates"):
        P, Q, _ = kn.set_rows(name)
        skip = np.full(len(Q), -1, np.int32)
        skip[::2] = np.arange(len(Q))[::2] * 5 % len(P)
        eng = _engine(P)
        for k in (5, 33, 64):
            for kw in ({}, {"skip_ids": skip}):
                a, b = eng.knn(Q, k, **kw), eng.radius_knn(Q, k, radius=4.0, **kw)
                assert np.array_equal(_np(a["idx"]), _np(b["idx"])) and np.array_equal(_np(a["counts"]), _np(b["counts"])), (name, k)
                assert np.array_equal(_np(a["dist"]).view(np.int32), _np(b["dist"]).view(np.int32)), (name, k)
                print("%s k=%d: point tests %d seeded (+ %d for the seeds), %d from radius 4" % (name, k, a["info"]["point_tests"], a["info"]["seed_point_tests"],
                                                                                                 b["info"]["point_tests"]))
        eng.close()


def test_self_mode_is_solve_plus_repair_exact():
    from owlraytracing_amd import datasets

    for name in ("uniform", "duplicates"):
        P = kn.set_self_rows(name)[0]
        eng = _engine(P)
        for k in (5, 17):
            r0 = datasets.start_radius(len(P), k)
            res = eng.solve(k, r0, want_levels=True)
            eng.repair_exact(res, k, r0)
            got = eng.knn(k=k)
            done = (_np(res["levels"]) >= 0) & np.isfinite(_np(res["dist"])).all(axis=1)
            assert done.sum() > len(P) // 2
            assert np.array_equal(_np(got["idx"])[done], _np(res["idx"])[done]), (name, k)
            assert np.array_equal(_np(got["dist"])[done].view(np.int32), _np(res["dist"])[done].view(np.int32)), (name, k)
        eng.close()


# ---- 8. side effects ---------------------------------------------------------------------------------------------------------------
def test_solve_state_halo_tree_and_radius_knn_are_left_alone():
    import torch

    P, Q = kn.lattice_case()
    rows = kn.rows_of(("lattice",), lambda: kn.knn_rows(P, Q, max(rk.LATTICE_K)))
    eng = _engine(P)
    before = eng.solve(5, 0.02)
    _same(eng.knn(Q, 6), kn.cut(rows, 6), "between two solves")
    eng.knn(k=6)
    after = eng.solve(5, 0.02)
    for key in ("idx", "dist", "intersections"):
        assert torch.equal(before[key], after[key]), key
    eng.set_halo(P[:50] + np.float32(0.001), np.arange(50, dtype=np.int32) + 5000)
    got = eng.knn(Q, 6)
    _same(got, kn.cut(rows, 6), "with a halo tree set")
    assert (_np(got["idx"]) < 5000).all()
    # tknnRadiusKnn keeps its own rule for a zero radius: refused as the call's radius, an empty row as a row's
    from owlraytracing_amd._lib import TknnError

    with pytest.raises(TknnError) as err:
        eng.radius_knn(Q, 6, radius=0.0)
    assert err.value.code == ARG
    radii = np.full(len(Q), 0.0, np.float32)
    radii[1::2] = np.float32(1.0 / 32)
    got = eng.radius_knn(Q, 6, radii=radii)
    _same({k: got[k] for k in ("idx", "dist", "counts")}, rk.knn_rows(P, Q, 6, radii=radii), "radii of zero")
    assert (_np(got["counts"])[0::2] == 0).all() and (_np(got["counts"])[1::2] > 0).any()
    assert (_np(got["counts"])[:200:2] == 0).all(), "node queries lie ON a point: a zero radius still is an empty row"
    eng.close()


# ---- 9. the Python front end -------------------------------------------------------------------------------------------------------
def test_python_front_end():
    import torch

    from owlraytracing_amd.trueknn import knn, knn_graph

    P, Q, rows = kn.set_rows("planar")
    want = kn.cut(rows, 17)
    res = knn(P, Q, 17)
    _same(res, want, "one-shot helper")
    assert res["build_info"]["n"] == len(P) and isinstance(res["idx"], np.ndarray)
    flat = np.ascontiguousarray(P[:600, :2])  # (n, 2): z = 0
    g = knn_graph(flat, 6)
    _same(g, kn.self_rows(flat, 6), "knn_graph")
    assert not (g["idx"] == np.arange(len(flat))[:, None]).any(), "no (i, i) entry"
    looped = knn_graph(flat, 6, loop=True)
    _same(looped, kn.knn_rows(flat, flat, 6), "knn_graph(loop=True)")
    assert (looped["idx"][:, 0] == np.arange(len(flat))).all() and (looped["dist"][:, 0] == 0).all()
    eng = _engine(P)
    _same(eng.knn(torch.from_numpy(np.array(Q)).cuda(), 17), want, "a device tensor")
    skip = torch.arange(len(Q), dtype=torch.int32).cuda()
    _same(eng.knn(Q, 17, skip_ids=skip), kn.knn_rows(P, Q, 17, skip=np.arange(len(Q))), "skip ids on the device")
    only_idx = eng.knn(Q, 17, want_dist=False)
    assert "dist" not in only_idx and np.array_equal(_np(only_idx["idx"]), want["idx"])
    eng.close()
