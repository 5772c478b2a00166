"""TrueKNN.periodic_knn (tknnPeriodicKnn: at most k nearest points under a per-axis periodic metric) against
tests/periodic_spec.py on a GPU: idx, dist and counts of every row, bit for bit.  n <= 4 096 except for the pyramid case.

| case      | P                                        | queries, k                                                                     |
|-----------|------------------------------------------|--------------------------------------------------------------------------------|
| uniform   | 2 000 in the cell (0.1, -0.3, 2) + (0.3, 0.7, open) | 300 external and its own points, every k of K_ALL; ids; skip_ids    |
| lattice   | spacing 1/16, unit cell, xyz periodic    | the x = 0 face's own rows, cell centres, edge midpoints; k = 1, 3, 6, 7; r = 1/16 |
| radii     | uniform                                  | r_j = the wrapped distance to a point across a face, and one ulp below         |
| tiny      | 1, 2, 16, 17, 65, 20 points              | k below, at and above n, both kernels: rows not full, d beyond half a period   |
| pyramid   | 70 000 uniform, unit cell                | 256 queries, half within 0.01 of a face; k = 10, 64                            |
| open      | uniform set of knn_spec                  | no periodic axis, a cell ten scene widths wide: knn's and radius_knn's rows    |
| fallback  | uniform, lattice                         | TKNN_PERIODIC_KNN_FORCE_FALLBACK=1: the one-query-per-lane kernel              |
| edge      | NaN points, 40 copies of one point       | queries outside the cell, NaN queries, NaN / inf / 0 radii                     |
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_spec as kn  # noqa: E402
import periodic_spec as ps  # noqa: E402

pytestmark = pytest.mark.gpu

FALLBACK = "TKNN_PERIODIC_KNN_FORCE_FALLBACK"


def _engine(P, ids=None):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(P, ids=ids)
    return eng


def _np(v):
    return np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v)


def _same(got, want, what, seeded=None):
    """The engine's dense rows equal the spec's: counts, indices, the distances' bits, the padding; no row holds an index twice;
    the info's sums are the rows'; seed_point_tests is 0 exactly when no seed pass ran (`seeded`, where given)."""
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
        assert 0 <= info["tightened_rows"] <= info["full_rows"] and 0 <= info["lane_rows"] <= len(idx), what
        if seeded is not None:
            assert (info["seed_point_tests"] > 0) == seeded, (what, info)


def _equal_rows(a, b, what):
    assert np.array_equal(_np(a["idx"]), _np(b["idx"])) and np.array_equal(_np(a["counts"]), _np(b["counts"])), what
    assert np.array_equal(_np(a["dist"]).view(np.int32), _np(b["dist"]).view(np.int32)), what


# ---- 1. uniform points in a non-dyadic cell -----------------------------------------------------------------------------------------
def _uniform_rows():
    P, Q, lo, period = ps.uniform_case()
    return (P, Q, lo, period, ps.rows_of(("uniform",), lambda: ps.knn_rows(P, Q, ps.K_MAX, lo, period)),
            ps.rows_of(("uniform-self",), lambda: ps.self_rows(P, ps.K_MAX, lo, period)))


def test_uniform_rows_equal_the_spec():
    P, Q, lo, period, rows, own = _uniform_rows()
    eng = _engine(P)
    for k in ps.K_ALL:
        got = eng.periodic_knn(Q, k, lo=lo, period=period)
        _same(got, ps.cut(rows, k), "uniform k=%d" % k, seeded=True)
        assert got["info"]["lane_rows"] == 0 and got["info"]["point_tests"] > 0 and got["info"]["node_tests"] > 0
        got = eng.periodic_knn(k=k, lo=lo, period=period)
        _same(got, ps.cut(own, k), "uniform self k=%d" % k, seeded=True)
        assert not (_np(got["idx"]) == np.arange(len(P))[:, None]).any(), "no row holds its own point"
    info = eng.periodic_knn(Q, 10, lo=lo, period=period)["info"]
    assert info["tightened_rows"] > 0 and info["solve_ms"] >= info["walk_ms"] > 0 and info["seed_ms"] > 0 and info["order_ms"] > 0
    eng.close()


def test_uniform_rows_with_ids_and_skips():
    import torch

    P, Q, lo, period, rows, own = _uniform_rows()
    ids = ps.uniform_ids(len(P))
    skip = np.full(len(Q), -1, np.int32)
    skip[::2] = rows["idx"][::2, 0]  # every other query skips its nearest point
    id_skip = np.where(skip >= 0, ids[np.maximum(skip, 0)], -1).astype(np.int32)
    want_skip = ps.rows_of(("uniform-skip",), lambda: ps.knn_rows(P, Q, ps.K_MAX, lo, period, skip=skip))
    want_ids = ps.rows_of(("uniform-ids",), lambda: ps.knn_rows(P, Q, ps.K_MAX, lo, period, ids=ids))
    want_id_skip = ps.rows_of(("uniform-id-skip",), lambda: ps.knn_rows(P, Q, ps.K_MAX, lo, period, skip=id_skip, ids=ids))
    want_own = ps.rows_of(("uniform-self-ids",), lambda: ps.self_rows(P, ps.K_MAX, lo, period, ids=ids))
    assert (want_skip["idx"][::2, 0] == rows["idx"][::2, 1]).all() and (want_ids["idx"] != rows["idx"]).any()
    eng = _engine(P)
    by_id = _engine(torch.from_numpy(np.array(P)).cuda(), torch.from_numpy(ids.copy()).cuda())
    for k in ps.K_ALL:
        _same(eng.periodic_knn(Q, k, lo=lo, period=period, skip_ids=skip), ps.cut(want_skip, k), "skip k=%d" % k)
        _same(by_id.periodic_knn(Q, k, lo=lo, period=period), ps.cut(want_ids, k), "ids k=%d" % k)
        _same(by_id.periodic_knn(Q, k, lo=lo, period=period, skip_ids=id_skip), ps.cut(want_id_skip, k), "skip by id k=%d" % k)
        got = by_id.periodic_knn(k=k, lo=lo, period=period)
        _same(got, ps.cut(want_own, k), "self by id k=%d" % k)
        assert not (_np(got["idx"]) == ids[:, None]).any()
    eng.close(), by_id.close()


def test_uniform_rows_within_a_radius():
    """A radius for all rows and one per row, external and by row in self mode: no seed pass, rows that are not full."""
    P, Q, lo, period, rows, own = _uniform_rows()
    r = np.float32(0.03)
    rng = np.random.default_rng(94)
    radii = (rng.random(len(Q), dtype=np.float32) * np.float32(0.06)).astype(np.float32)
    own_radii = (rng.random(len(P), dtype=np.float32) * np.float32(0.06)).astype(np.float32)
    eng = _engine(P)
    for k in (5, 16, 33):
        want = ps.knn_rows(P, Q, k, lo, period, radius=r)
        assert (want["counts"] < k).any() and ((want["counts"] == k).any() or k > 5)
        _same(eng.periodic_knn(Q, k, lo=lo, period=period, radius=r), want, "radius k=%d" % k, seeded=False)
        _same(eng.periodic_knn(Q, k, lo=lo, period=period, radii=radii), ps.knn_rows(P, Q, k, lo, period, radii=radii), "radii k=%d" % k, seeded=False)
        _same(eng.periodic_knn(k=k, lo=lo, period=period, radius=r), ps.self_rows(P, k, lo, period, radius=r), "self radius k=%d" % k, seeded=False)
        _same(eng.periodic_knn(k=k, lo=lo, period=period, radii=own_radii), ps.self_rows(P, k, lo, period, radii=own_radii), "self radii k=%d" % k,
              seeded=False)
    eng.close()


# ---- 2. lattice ------------------------------------------------------------------------------------------------------------------------
def test_lattice_rows_across_the_faces():
    P, Q, face = ps.lattice_case()
    lo, period = ps.UNIT
    kmax = max(ps.LATTICE_K)
    rows = ps.rows_of(("lattice",), lambda: ps.knn_rows(P, Q, kmax, lo, period))
    own = ps.rows_of(("lattice-self",), lambda: ps.self_rows(P, kmax, lo, period))
    eng = _engine(P)
    for k in ps.LATTICE_K:
        _same(eng.periodic_knn(Q, k, lo=lo, period=period), ps.cut(rows, k), "lattice k=%d" % k)
        got = eng.periodic_knn(k=k, lo=lo, period=period)
        _same(got, ps.cut(own, k), "lattice self k=%d" % k)
        assert (_np(got["dist"])[face, 0] == ps.LATTICE_SPACING).all(), "the x = 0 face's nearest points are one spacing away"
    # a radius of exactly the spacing: six neighbours exactly at r, three of them across a face for the corner point
    r = ps.LATTICE_SPACING
    got = eng.periodic_knn(k=7, lo=lo, period=period, radius=float(r))
    _same(got, ps.self_rows(P, 7, lo, period, radius=r), "lattice r = 1/16", seeded=False)
    assert (_np(got["counts"]) == 6).all() and (_np(got["dist"])[:, :6] == r).all()
    corner = np.zeros((1, 3), np.float32)
    _same(eng.periodic_knn(corner, 7, lo=lo, period=period, radius=float(r)), ps.knn_rows(P, corner, 7, lo, period, radius=r), "the corner at r = 1/16")
    eng.close()


# ---- 3. exact radii across a face --------------------------------------------------------------------------------------------------------
def test_exact_radii_across_a_face():
    P, Q, lo, period, rows, own = _uniform_rows()
    d = ps.wrapped(P, Q, lo, period)
    crossing = d.view(np.int32) != ps.wrapped(P, Q, lo, period, wrap=False).view(np.int32)
    ranked = np.argsort(np.where(crossing, d, np.inf), axis=1, kind="stable")
    target = ranked[np.arange(len(Q)), np.arange(len(Q)) % 4]  # the nearest, second .. fourth nearest point across a face
    radii = d[np.arange(len(Q)), target]
    assert crossing[np.arange(len(Q)), target].all() and np.isfinite(radii).all() and (radii > 0).all()
    below = np.nextafter(radii, np.float32(0))
    k = 64
    want, want_below = ps.knn_rows(P, Q, k, lo, period, radii=radii), ps.knn_rows(P, Q, k, lo, period, radii=below)
    sharp = want["counts"] < k  # rows the radius cuts, not k: the last entry lies at r_j
    assert sharp.mean() > 0.3 and (want["idx"][sharp] == target[sharp, None]).any(axis=1).all()
    assert not (want_below["idx"] == target[:, None]).any()
    eng = _engine(P)
    got = eng.periodic_knn(Q, k, lo=lo, period=period, radii=radii)
    _same(got, want, "r_j = the distance to a point across a face", seeded=False)
    assert (_np(got["idx"])[sharp] == target[sharp, None]).any(axis=1).all(), "a distance exactly r_j is inside"
    got = eng.periodic_knn(Q, k, lo=lo, period=period, radii=below)
    _same(got, want_below, "one ulp below", seeded=False)
    assert not (_np(got["idx"]) == target[:, None]).any()
    eng.close()


# ---- 4. tiny sets ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ps.TINY_N)
def test_tiny_sets(n, monkeypatch):
    """Under the team walk (a pyramid of one level) and, forced, under the lane kernel: rows that are not full, distances beyond
    half a period, no point twice."""
    P, Q, ks = ps.tiny_case(n)
    lo, period = ps.UNIT
    eng = _engine(P)
    for forced in (False, True):
        if forced:
            monkeypatch.setenv(FALLBACK, "1")
        for k in ks:
            got = eng.periodic_knn(Q, k, lo=lo, period=period)
            _same(got, ps.knn_rows(P, Q, k, lo, period), "n=%d k=%d forced=%d" % (n, k, forced))
            assert got["info"]["lane_rows"] == (len(Q) if forced else 0)
            if k > n:
                assert got["info"]["full_rows"] == 0
            if k >= n:
                assert (_np(got["dist"])[:, :n].max(axis=1) > 0.5).all(), "a distance beyond half a period"
            _same(eng.periodic_knn(k=k, lo=lo, period=period), ps.self_rows(P, k, lo, period), "self n=%d k=%d forced=%d" % (n, k, forced))
    monkeypatch.delenv(FALLBACK)
    eng.close()


# ---- 5. a pyramid of three levels ----------------------------------------------------------------------------------------------------------
def test_a_pyramid_of_three_levels():
    P, Q = ps.pyramid_case()
    lo, period = ps.UNIT
    rows = ps.rows_of(("pyramid",), lambda: ps.knn_rows(P, Q, ps.K_MAX, lo, period, block=32))
    eng = _engine(P)
    assert eng.export_tree_ex()["wide_levels"] == 3
    for k in (10, 64):
        got = eng.periodic_knn(Q, k, lo=lo, period=period)
        _same(got, ps.cut(rows, k), "pyramid k=%d" % k, seeded=True)
        assert got["info"]["lane_rows"] == 0 and got["info"]["full_rows"] == len(Q)
        assert got["info"]["point_tests"] < len(Q) * len(P) // 20, "the gate prunes: far fewer point tests than brute force"
    eng.close()


# ---- 6. no periodic axis, a large cell: the existing calls ---------------------------------------------------------------------------------
def test_open_axes_and_a_large_cell_give_the_existing_rows():
    P, Q, rows = kn.set_rows("uniform")
    width = float((P.max(0) - P.min(0)).max())
    mid = (P.max(0) + P.min(0)) / 2
    cells = (((0, 0, 0), (0, 0, 0)), (tuple(float(v) for v in mid - 5 * width), (10 * width,) * 3))
    skip = np.full(len(Q), -1, np.int32)
    skip[::3] = np.arange(len(Q))[::3] * 7 % len(P)
    eng = _engine(P)
    for lo, period in cells:
        for k in (5, 33, 64):
            for kw in ({}, {"skip_ids": skip}):
                _equal_rows(eng.periodic_knn(Q, k, lo=lo, period=period, **kw), eng.knn(Q, k, **kw), ("knn", period, k))
                _equal_rows(eng.periodic_knn(Q, k, lo=lo, period=period, radius=0.07, **kw), eng.radius_knn(Q, k, radius=0.07, **kw), ("radius_knn", period, k))
            _equal_rows(eng.periodic_knn(k=k, lo=lo, period=period), eng.knn(k=k), ("self", period, k))
            _same(eng.periodic_knn(Q, k, lo=lo, period=period), kn.cut(rows, k), "open k=%d" % k)
    eng.close()


# ---- 7. forced fallback ----------------------------------------------------------------------------------------------------------------------
def test_forced_fallback_gives_identical_rows(monkeypatch):
    """TKNN_PERIODIC_KNN_FORCE_FALLBACK=1 (read per call): the walk leaves every query to the one-query-per-lane kernel."""
    P, Q, lo, period, rows, own = _uniform_rows()
    LP, LQ, _ = ps.lattice_case()
    lattice = ps.rows_of(("lattice",), lambda: ps.knn_rows(LP, LQ, max(ps.LATTICE_K), ps.UNIT[0], ps.UNIT[1]))
    for name, P_, Q_, cell, want, ks in (("uniform", P, Q, (lo, period), rows, (1, 16, 17, 64)), ("lattice", LP, LQ, ps.UNIT, lattice, ps.LATTICE_K)):
        eng = _engine(P_)
        for k in ks:
            for kw in ({}, {"radius": 0.0625}):
                plain = eng.periodic_knn(Q_, k, lo=cell[0], period=cell[1], **kw)
                plain_own = eng.periodic_knn(k=k, lo=cell[0], period=cell[1], **kw)
                monkeypatch.setenv(FALLBACK, "1")
                forced = eng.periodic_knn(Q_, k, lo=cell[0], period=cell[1], **kw)
                forced_own = eng.periodic_knn(k=k, lo=cell[0], period=cell[1], **kw)
                monkeypatch.delenv(FALLBACK)
                assert plain["info"]["lane_rows"] == 0 and forced["info"]["lane_rows"] == len(Q_) and forced_own["info"]["lane_rows"] == len(P_)
                if not kw:
                    _same(forced, ps.cut(want, k), "fallback %s k=%d" % (name, k), seeded=True)
                for a, b in ((plain, forced), (plain_own, forced_own)):
                    _equal_rows(a, b, (name, k, kw))
                    assert a["info"]["total"] == b["info"]["total"] and a["info"]["full_rows"] == b["info"]["full_rows"]
                    assert a["info"]["tightened_rows"] == b["info"]["tightened_rows"]
        eng.close()


# ---- 8. edge inputs ----------------------------------------------------------------------------------------------------------------------------
def test_edge_inputs():
    P, Q, radii = ps.edge_case()
    lo, period = ps.CELL
    nan_p = np.flatnonzero(np.isnan(P).any(axis=1))
    eng = _engine(P)
    for k in (1, 16, 40, 41, 64):
        got = eng.periodic_knn(Q, k, lo=lo, period=period)
        _same(got, ps.knn_rows(P, Q, k, lo, period), "edge k=%d" % k, seeded=True)
        assert (_np(got["counts"])[[1, 2, 3, 4, 7, 8, 9]] == 0).all(), "outside the cell or with a NaN: an empty row"
        assert (_np(got["counts"])[[0, 5, 6, 10]] == k).all() and not np.isin(_np(got["idx"]), nan_p).any()
        if k <= 40:
            assert _np(got["dist"])[0, k - 1] == 0, "k copies of the query: a seed bound of 0"
        _same(eng.periodic_knn(Q, k, lo=lo, period=period, radii=radii), ps.knn_rows(P, Q, k, lo, period, radii=radii), "edge radii k=%d" % k, seeded=False)
        own = eng.periodic_knn(k=k, lo=lo, period=period)
        _same(own, ps.self_rows(P, k, lo, period), "edge self k=%d" % k)
        assert (_np(own["counts"])[nan_p] == 0).all()
    eng.close()


# ---- 9. info, side effects, the front end ----------------------------------------------------------------------------------------------------------
def test_info_and_query_count_edges(monkeypatch):
    P, Q, lo, period, rows, own = _uniform_rows()
    eng = _engine(P)
    for m in (1, 2, 3, 4, 5, 63, 64, 65):
        _same(eng.periodic_knn(Q[:m], 5, lo=lo, period=period), ps.cut({k: v[:m] for k, v in rows.items()}, 5), "m=%d" % m, seeded=True)
    got = eng.periodic_knn(Q, 17, lo=lo, period=period)
    assert got["info"]["seed_point_tests"] == 3 * 16 * len(Q), "three blocks of 16 around every query for k = 17"
    assert got["info"]["total"] == int(_np(got["counts"]).sum()) and got["info"]["full_rows"] == int((_np(got["counts"]) == 17).sum())
    assert eng.periodic_knn(Q, 17, lo=lo, period=period, radius=0.05)["info"]["seed_point_tests"] == 0
    monkeypatch.setenv(FALLBACK, "1")
    assert eng.periodic_knn(Q, 17, lo=lo, period=period)["info"]["lane_rows"] == len(Q)
    assert eng.periodic_knn(k=3, lo=lo, period=period, radius=0.05)["info"]["lane_rows"] == len(P)
    monkeypatch.delenv(FALLBACK)
    empty = eng.periodic_knn(np.zeros((0, 3), np.float32), 5, lo=lo, period=period)
    assert empty["idx"].shape == (0, 5) and empty["counts"].shape == (0,)
    assert empty["info"]["total"] == 0 and empty["info"]["solve_ms"] == 0 and empty["info"]["node_tests"] == 0
    eng.close()


def test_solve_state_and_halo_tree_are_left_alone():
    import torch

    P, Q, lo, period, rows, own = _uniform_rows()
    eng = _engine(P)
    before = eng.solve(5, 0.02)
    knn_before = eng.knn(Q, 6)
    _same(eng.periodic_knn(Q, 6, lo=lo, period=period), ps.cut(rows, 6), "between two solves")
    eng.periodic_knn(k=6, lo=lo, period=period)
    after = eng.solve(5, 0.02)
    for key in ("idx", "dist", "intersections"):
        assert torch.equal(before[key], after[key]), key
    _equal_rows(knn_before, eng.knn(Q, 6), "tknnKnn before and after")
    eng.set_halo(P[:50] + np.float32(0.001), np.arange(50, dtype=np.int32) + 5000)
    got = eng.periodic_knn(Q, 6, lo=lo, period=period)
    _same(got, ps.cut(rows, 6), "with a halo tree set")
    assert (_np(got["idx"]) < 5000).all()
    eng.close()


def test_python_front_end():
    import torch

    P, Q, lo, period, rows, own = _uniform_rows()
    want = ps.cut(rows, 17)
    eng = _engine(P)
    _same(eng.periodic_knn(torch.from_numpy(np.array(Q)).cuda(), 17, lo=tuple(lo), period=tuple(period)), want, "a device tensor, tuples")
    only_idx = eng.periodic_knn(Q, 17, lo=lo, period=period, want_dist=False)
    assert "dist" not in only_idx and np.array_equal(_np(only_idx["idx"]), want["idx"])
    flat, flat_q = np.ascontiguousarray(P[:, :2]), np.ascontiguousarray(Q[:, :2])  # (n, 2): z = 0, two periods
    plane = _engine(flat)
    _same(plane.periodic_knn(flat_q, 6, lo=lo[:2], period=period[:2]), ps.knn_rows(flat, flat_q, 6, np.float32([lo[0], lo[1], 0]), np.float32([period[0], period[1], 0])),
          "2-D data")
    plane.close()
    for kw in ({}, {"period": period, "radius": 0.1, "radii": np.ones(len(Q), np.float32)}, {"period": (1, 2, 3, 4)}, {"period": period, "lo": (1,) * 4}):
        with pytest.raises(ValueError):
            eng.periodic_knn(Q, 5, **kw)
    with pytest.raises(ValueError):
        eng.periodic_knn(k=5, period=period, lo=lo, skip_ids=np.zeros(len(P), np.int32))
    with pytest.raises(ValueError):
        eng.periodic_knn(Q, 5, period=period, lo=lo, radii=np.ones(len(Q) - 1, np.float32))
    eng.close()
