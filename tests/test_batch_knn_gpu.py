"""TrueKNN.batch_knn (tknnBatchKnn: at most k nearest points inside the query's own batch) against tests/batch_spec.py on a GPU:
idx, dist and counts of every row, bit for bit, for external queries and for the set's own points, under the team walk and,
with TKNN_BATCH_KNN_FORCE_FALLBACK=1, under the one-query-per-lane kernel.  Nothing exceeds 20 000 points.

| case    | P                                                            | queries, k                                              |
|---------|--------------------------------------------------------------|---------------------------------------------------------|
| small   | 10 points, 3 batches                                         | k = 4: below, at and above the batches' sizes           |
| clouds  | 3 000: seven overlapping unit-cube clouds of 0 .. 1 500      | 30 per label and its own points, k = 1, 10, 16, 17, 64  |
| range   | clouds                                                       | only the 5- and 40-point batches: the walk's work bound |
| large   | 20 000 uniform, 33 and 4 096 batches                         | 256 external, a sample of its own rows; k = 10, 33      |
| twins   | the same coordinates in two batches                          | those coordinates under each label                      |
| ids     | clouds with ids                                              | skip_ids by id, its own rows by id                      |
| planar  | clouds, (n, 2)                                               | 2-D queries                                             |
| edge    | NaN points, NaN queries, labels no batch has                 | one radius, per-row radii with NaN, inf, 0, FLT_MAX     |
| one     | one batch                                                    | tknnKnn's and tknnRadiusKnn's rows                      |
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_spec as bs  # noqa: E402

pytestmark = pytest.mark.gpu

FALLBACK = "TKNN_BATCH_KNN_FORCE_FALLBACK"


def _engine(P, batch, num_batches=None, ids=None):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(P, ids=ids, batch=batch, num_batches=num_batches)
    return eng


def _np(v):
    return np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v)


def _same(got, want, what, seeded=None, rows=None):
    """The engine's dense rows (or those of ``rows``) equal the spec's: counts, indices, the distances' bits, the padding; no row
    holds an index twice; the info's sums are the rows'; seed_point_tests is 0 exactly when no seed pass ran."""
    idx, dist, counts = _np(got["idx"]), _np(got["dist"]), _np(got["counts"])
    assert idx.dtype == np.int32 and dist.dtype == np.float32 and counts.dtype == np.int32
    if rows is not None:
        idx, dist, counts = idx[rows], dist[rows], counts[rows]
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
    if "info" in got and rows is None:
        info = got["info"]
        assert info["total"] == want["counts"].sum() and info["full_rows"] == (want["counts"] == idx.shape[1]).sum(), what
        assert 0 <= info["tightened_rows"] <= info["full_rows"] and 0 <= info["lane_rows"] <= len(idx), what
        if seeded is not None:
            assert (info["seed_point_tests"] > 0) == seeded, (what, info)


def _both_paths(monkeypatch, eng, call, want, what, m, **same_kw):
    """``call()`` under the team walk (no row left to the lane kernel) and under the forced fallback (every row)."""
    for forced in (False, True):
        if forced:
            monkeypatch.setenv(FALLBACK, "1")
        try:
            got = call()
        finally:
            if forced:
                monkeypatch.delenv(FALLBACK)
        _same(got, want, "%s forced=%d" % (what, forced), **same_kw)
        assert got["info"]["lane_rows"] == (m if forced else 0), (what, forced, got["info"])


# ---- 1. ten points ----------------------------------------------------------------------------------------------------------------------
def test_ten_points_in_three_batches(monkeypatch):
    rng = np.random.default_rng(371)
    P = rng.random((10, 3), dtype=np.float32)
    batch = np.int32([2, 0, 1, 0, 0, 2, 0, 1, 0, 0])  # sizes 6, 2, 2
    Q = rng.random((9, 3), dtype=np.float32)
    bq = np.int32([0, 1, 2, 0, 1, 2, 0, 1, 2])
    eng = _engine(P, batch)
    for k in (1, 4, 6):
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(Q, k, batch=bq), bs.knn_rows(P, batch, Q, bq, k), "small k=%d" % k, len(Q), seeded=True)
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(k=k), bs.self_rows(P, batch, k), "small self k=%d" % k, len(P), seeded=True)
    got = eng.batch_knn(k=4)
    assert _np(got["counts"]).tolist() == [1, 4, 1, 4, 4, 1, 4, 1, 4, 4], "k may exceed the size of a batch"
    eng.close()


# ---- 2. seven overlapping clouds ------------------------------------------------------------------------------------------------------------
def _clouds():
    P, batch, Q, bq = bs.clouds_case()
    return (P, batch, Q, bq, bs.rows_of(("clouds",), lambda: bs.knn_rows(P, batch, Q, bq, bs.K_MAX)),
            bs.rows_of(("clouds-self",), lambda: bs.self_rows(P, batch, bs.K_MAX)))


@pytest.mark.parametrize("k", [1, 10, 16, 17, 64])
def test_seven_overlapping_clouds(k, monkeypatch):
    P, batch, Q, bq, rows, own = _clouds()
    eng = _engine(P, batch)
    _both_paths(monkeypatch, eng, lambda: eng.batch_knn(Q, k, batch=bq), bs.cut(rows, k), "clouds k=%d" % k, len(Q), seeded=True)
    _both_paths(monkeypatch, eng, lambda: eng.batch_knn(k=k), bs.cut(own, k), "clouds self k=%d" % k, len(P), seeded=True)
    got = eng.batch_knn(Q, k, batch=bq)
    idx = _np(got["idx"])
    assert (batch[idx[idx >= 0]] == np.broadcast_to(bq[:, None], idx.shape)[idx >= 0]).all(), "every entry carries the query's label"
    assert (_np(got["counts"]) == np.minimum(k, np.array(bs.CLOUD_SIZES)[bq])).all()
    own_idx = _np(eng.batch_knn(k=k)["idx"])
    assert not (own_idx == np.arange(len(P))[:, None]).any(), "no row holds its own point"
    info = got["info"]
    assert info["solve_ms"] >= info["walk_ms"] > 0 and info["seed_ms"] > 0 and info["order_ms"] > 0 and info["node_tests"] > 0
    eng.close()


def test_the_walk_reads_only_blocks_that_touch_the_batch():
    """The range rule as a condition: with no radius and queries in the 5-point and the 40-point batch only, every block the
    walk reads touches the query's slot range [s, e), and no row is left to the lane kernel.  A walk that filtered only at
    the leaf would test all 3 000 points for the queries whose seed bound is FLT_MAX."""
    P, batch, Q, bq, rows, own = _clouds()
    pick = np.flatnonzero((bq == 2) | (bq == 3))
    Q2, bq2 = np.ascontiguousarray(Q[pick]), np.ascontiguousarray(bq[pick])
    eng = _engine(P, batch)
    starts = _np(eng.batch_layout()["starts"]).astype(np.int64)
    assert np.array_equal(np.diff(starts), bs.CLOUD_SIZES)
    s, e = starts[bq2], starts[bq2 + 1]
    touching = (e - 1) // 16 - s // 16 + 1
    for k in (10, 64):
        got = eng.batch_knn(Q2, k, batch=bq2)
        _same(got, bs.cut({name: v[pick] for name, v in rows.items()}, k), "range k=%d" % k, seeded=True)
        info = got["info"]
        print("k=%d: point_tests %d (bound %d), seed_point_tests %d (bound %d), lane_rows %d, node_tests %d"
              % (k, info["point_tests"], 16 * touching.sum(), info["seed_point_tests"], 16 * len(Q2) * ((k + 15) // 16 + 1), info["lane_rows"], info["node_tests"]))
        assert info["lane_rows"] == 0
        assert info["point_tests"] <= 16 * touching.sum()
        assert info["seed_point_tests"] <= 16 * len(Q2) * ((k + 15) // 16 + 1)
        assert info["point_tests"] > 0 and info["seed_point_tests"] > 0
    eng.close()


# ---- 3. 20 000 points in 33 and in 4 096 batches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_batches", [33, 4096])
def test_twenty_thousand_points(num_batches, monkeypatch):
    P, batch, Q, bq = bs.large_case(num_batches)
    sample = np.random.default_rng(372).choice(len(P), 300, replace=False)
    eng = _engine(P, batch, num_batches)
    assert eng.export_tree_ex()["wide_levels"] == 2
    for k in (10, 33):
        want = bs.knn_rows(P, batch, Q, bq, k)
        assert (want["counts"][[5, 9, 77, 200]] == 0).all()
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(Q, k, batch=bq), want, "B=%d k=%d" % (num_batches, k), len(Q), seeded=True)
        want_own = bs.knn_rows(P, batch, P[sample], batch[sample], k, skip=sample)
        assert (want_own["counts"] == np.minimum(k, np.bincount(batch, minlength=num_batches)[batch[sample]] - 1)).all()
        assert (want_own["counts"] < k).any() == (num_batches == 4096), "small batches: rows that are not full"
        for forced in (False, True):
            if forced:
                monkeypatch.setenv(FALLBACK, "1")
            got = eng.batch_knn(k=k)
            if forced:
                monkeypatch.delenv(FALLBACK)
            _same(got, want_own, "B=%d self k=%d forced=%d" % (num_batches, k, forced), rows=sample)
            assert got["info"]["lane_rows"] == (len(P) if forced else 0)
            idx = _np(got["idx"])
            assert (batch[idx[idx >= 0]] == np.broadcast_to(batch[:, None], idx.shape)[idx >= 0]).all()
            assert (_np(got["counts"]) == np.minimum(k, np.bincount(batch, minlength=num_batches)[batch] - 1)).all()
    eng.close()


# ---- 4. the same coordinates in two batches ----------------------------------------------------------------------------------------------------
def test_the_same_coordinates_in_two_batches(monkeypatch):
    P, batch, Q, bq = bs.twins_case()
    eng = _engine(P, batch)
    for k in (1, 2, 17):
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(Q, k, batch=bq), bs.knn_rows(P, batch, Q, bq, k), "twins k=%d" % k, len(Q))
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(k=k), bs.self_rows(P, batch, k), "twins self k=%d" % k, len(P))
    got = eng.batch_knn(Q, 1, batch=bq)
    assert (_np(got["dist"])[:80, 0] == 0).all() and (batch[_np(got["idx"])[:80, 0]] == bq[:80]).all(), "each label finds its own copy"
    assert (_np(eng.batch_knn(k=1)["dist"])[batch < 2, 0] > 0).all(), "the twin in the other batch is no neighbour"
    eng.close()


# ---- 5. ids, skips, 2-D data --------------------------------------------------------------------------------------------------------------------
def test_ids_and_skips(monkeypatch):
    import torch

    P, batch, Q, bq, rows, own = _clouds()
    ids = ((np.arange(len(P), dtype=np.int64) * 7919) % 100003 + 5).astype(np.int32)
    assert len(set(ids.tolist())) == len(P)
    skip = np.full(len(Q), -1, np.int32)
    skip[::2] = rows["idx"][::2, 0]  # every other query skips its nearest point (-1 where its batch is empty)
    id_skip = np.where(skip >= 0, ids[np.maximum(skip, 0)], -1).astype(np.int32)
    eng = _engine(P, batch)
    by_id = _engine(torch.from_numpy(np.array(P)).cuda(), torch.from_numpy(batch.copy()).cuda(), ids=torch.from_numpy(ids.copy()).cuda())
    for k in (5, 17):
        want = bs.knn_rows(P, batch, Q, bq, k, skip=skip)
        full = rows["counts"][::2] >= 2
        assert (want["idx"][::2, 0][full] == rows["idx"][::2, 1][full]).all()
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(Q, k, batch=bq, skip_ids=skip), want, "skip k=%d" % k, len(Q))
        _both_paths(monkeypatch, by_id, lambda: by_id.batch_knn(Q, k, batch=bq), bs.knn_rows(P, batch, Q, bq, k, ids=ids), "ids k=%d" % k, len(Q))
        _both_paths(monkeypatch, by_id, lambda: by_id.batch_knn(Q, k, batch=bq, skip_ids=id_skip), bs.knn_rows(P, batch, Q, bq, k, skip=id_skip, ids=ids),
                    "skip by id k=%d" % k, len(Q))
        _both_paths(monkeypatch, by_id, lambda: by_id.batch_knn(k=k), bs.self_rows(P, batch, k, ids=ids), "self by id k=%d" % k, len(P))
        assert not (_np(by_id.batch_knn(k=k)["idx"]) == ids[:, None]).any()
    eng.close(), by_id.close()


def test_two_dimensional_data(monkeypatch):
    P, batch, Q, bq, rows, own = _clouds()
    flat, flat_q = np.ascontiguousarray(P[:, :2]), np.ascontiguousarray(Q[:, :2])
    eng = _engine(flat, batch)
    for k in (6, 20):
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(flat_q, k, batch=bq), bs.knn_rows(flat, batch, flat_q, bq, k), "2-D k=%d" % k, len(Q))
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(k=k), bs.self_rows(flat, batch, k), "2-D self k=%d" % k, len(P))
    eng.close()


# ---- 6. radii, NaN on either side, labels no batch has ----------------------------------------------------------------------------------------------
def test_radii_nan_and_labels_without_a_batch(monkeypatch):
    P, batch, Q, bq, radii = bs.nan_case()
    nan_p = np.flatnonzero(np.isnan(P).any(axis=1))
    own_radii = (np.random.default_rng(373).random(len(P), dtype=np.float32) * np.float32(0.3)).astype(np.float32)
    own_radii[[4, 5, 6]] = (np.nan, 0, np.inf)
    eng = _engine(P, batch, 4)
    for k in (1, 16, 64):
        want = bs.knn_rows(P, batch, Q, bq, k)
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(Q, k, batch=bq), want, "edge k=%d" % k, len(Q), seeded=True)
        assert (want["counts"][[1, 20, 41, 62, 3, 17, 18, 40, 63]] == 0).all() and not np.isin(want["idx"], nan_p).any()
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(Q, k, batch=bq, radii=radii), bs.knn_rows(P, batch, Q, bq, k, radii=radii), "edge radii k=%d" % k,
                    len(Q), seeded=False)
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(Q, k, batch=bq, radius=0.15), bs.knn_rows(P, batch, Q, bq, k, radius=np.float32(0.15)),
                    "edge radius k=%d" % k, len(Q), seeded=False)
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(k=k), bs.self_rows(P, batch, k), "edge self k=%d" % k, len(P), seeded=True)
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(k=k, radii=own_radii), bs.self_rows(P, batch, k, radii=own_radii), "edge self radii k=%d" % k,
                    len(P), seeded=False)
        _both_paths(monkeypatch, eng, lambda: eng.batch_knn(k=k, radius=0.1), bs.self_rows(P, batch, k, radius=np.float32(0.1)), "edge self radius k=%d" % k,
                    len(P), seeded=False)
        assert (_np(eng.batch_knn(k=k)["counts"])[nan_p] == 0).all()
    eng.close()


def test_exact_radii(monkeypatch):
    """r_j = the distance to a point of the batch: a distance exactly r_j is inside, one ulp below it is not."""
    P, batch, Q, bq, rows, own = _clouds()
    ok = np.flatnonzero(rows["counts"] >= 5)
    Q2, bq2 = np.ascontiguousarray(Q[ok]), np.ascontiguousarray(bq[ok])
    radii = np.ascontiguousarray(rows["dist"][ok, 4])
    target = rows["idx"][ok, 4]
    eng = _engine(P, batch)
    got = eng.batch_knn(Q2, 64, batch=bq2, radii=radii)
    _same(got, bs.knn_rows(P, batch, Q2, bq2, 64, radii=radii), "r_j = a point's distance", seeded=False)
    assert (_np(got["counts"]) == 5).all() and (_np(got["idx"])[:, 4] == target).all()
    below = np.nextafter(radii, np.float32(0))
    got = eng.batch_knn(Q2, 64, batch=bq2, radii=below)
    _same(got, bs.knn_rows(P, batch, Q2, bq2, 64, radii=below), "one ulp below", seeded=False)
    assert (_np(got["counts"]) == 4).all()
    eng.close()


# ---- 7. one batch: the unbatched calls ------------------------------------------------------------------------------------------------------------
def test_one_batch_gives_the_unbatched_rows():
    P, _, Q, _, _, _ = _clouds()
    zeros_p, zeros_q = np.zeros(len(P), np.int32), np.zeros(len(Q), np.int32)
    skip = np.full(len(Q), -1, np.int32)
    skip[::3] = np.arange(len(Q))[::3] * 7 % len(P)
    eng = _engine(P, zeros_p, 1)
    for k in (1, 16, 17, 64):
        for a, b in ((eng.batch_knn(Q, k, batch=zeros_q), eng.knn(Q, k)), (eng.batch_knn(Q, k, batch=zeros_q, skip_ids=skip), eng.knn(Q, k, skip_ids=skip)),
                     (eng.batch_knn(k=k), eng.knn(k=k)), (eng.batch_knn(Q, k, batch=zeros_q, radius=0.07), eng.radius_knn(Q, k, radius=0.07))):
            for name in ("idx", "dist", "counts"):
                assert np.array_equal(_np(a[name]).view(np.int32), _np(b[name]).view(np.int32)), (k, name)
    eng.close()


# ---- 8. info, side effects, the front end -------------------------------------------------------------------------------------------------------------
def test_info_and_query_count_edges(monkeypatch):
    P, batch, Q, bq, rows, own = _clouds()
    eng = _engine(P, batch)
    for m in (1, 2, 3, 4, 5, 63, 64, 65):
        part = slice(1, 1 + m)  # (query 0 is in the empty batch: alone it has no seeds)
        _same(eng.batch_knn(Q[part], 5, batch=bq[part]), bs.cut({k: v[part] for k, v in rows.items()}, 5), "m=%d" % m, seeded=True)
    assert eng.batch_knn(Q[:1], 5, batch=bq[:1])["info"]["seed_point_tests"] == 0, "an empty batch has no window"
    assert eng.batch_knn(Q, 17, batch=bq, radius=0.05)["info"]["seed_point_tests"] == 0
    empty = eng.batch_knn(np.zeros((0, 3), np.float32), 5, batch=np.zeros(0, np.int32))
    assert empty["idx"].shape == (0, 5) and empty["counts"].shape == (0,)
    assert empty["info"]["total"] == 0 and empty["info"]["solve_ms"] == 0 and empty["info"]["node_tests"] == 0
    eng.close()


def test_solve_state_and_halo_tree_are_left_alone():
    import torch

    P, batch, Q, bq, rows, own = _clouds()
    eng = _engine(P, batch)
    before = eng.solve(5, 0.05)
    _same(eng.batch_knn(Q, 6, batch=bq), bs.cut(rows, 6), "between two solves")
    eng.batch_knn(k=6)
    after = eng.solve(5, 0.05)
    for key in ("idx", "dist", "intersections"):
        assert torch.equal(before[key], after[key]), key
    eng.set_halo(P[:50] + np.float32(0.001), np.arange(50, dtype=np.int32) + 5000)
    got = eng.batch_knn(Q, 6, batch=bq)
    _same(got, bs.cut(rows, 6), "with a halo tree set")
    assert (_np(got["idx"]) < 5000).all()
    eng.close()


def test_python_front_end():
    import torch

    from owlraytracing_amd import trueknn

    P, batch, Q, bq, rows, own = _clouds()
    want = bs.cut(rows, 17)
    eng = _engine(P, batch)
    _same(eng.batch_knn(torch.from_numpy(np.array(Q)).cuda(), 17, batch=torch.from_numpy(bq.copy()).cuda()), want, "device tensors")
    only_idx = eng.batch_knn(Q, 17, batch=bq, want_dist=False)
    assert "dist" not in only_idx and np.array_equal(_np(only_idx["idx"]), want["idx"])
    for args, kw in (((Q, 5), {}), ((None, 5), {"batch": bq}), ((Q, 5), {"batch": bq[:-1]}), ((Q, 5), {"batch": bq, "radius": 0.1, "radii": np.ones(len(Q), np.float32)}),
                     ((None, 5), {"skip_ids": np.zeros(len(P), np.int32)}), ((Q, 5), {"batch": bq, "radii": np.ones(len(Q) - 1, np.float32)})):
        with pytest.raises(ValueError):
            eng.batch_knn(*args, **kw)
    with pytest.raises(ValueError):
        eng.build(P, num_batches=3)
    eng.close()
    _same(trueknn.batch_knn(P, batch, Q, bq, 17), want, "the one-shot")
    graph = trueknn.batch_knn_graph(P, batch, 6)
    _same(graph, bs.cut(own, 6), "batch_knn_graph")
    looped = trueknn.batch_knn_graph(P, batch, 6, loop=True)
    assert (looped["idx"][:, 0] == np.arange(len(P))).all() and (looped["dist"][:, 0] == 0).all()
    assert np.array_equal(looped["idx"][:, 1:], graph["idx"][:, :5])
