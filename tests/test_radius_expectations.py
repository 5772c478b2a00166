"""What the GPU tests of tknnRadiusQuery expect (tests/radius_spec.py), checked on the CPU: the brute-force rows against the
committed RT-DBSCAN oracle's counts, against a float64 kd-tree ball query away from the boundary, and the inputs of the boundary
and chunk-edge cases against what they claim to hold.  Runs without a GPU."""
import os
import sys

import numpy as np
import pytest
from scipy.spatial import cKDTree

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import dbscan_query_spec as ds  # noqa: E402
import query_spec as qs  # noqa: E402
import radius_spec as rs  # noqa: E402

import oracle  # noqa: E402


def _rows(rows, j):
    return rows["idx"][rows["offsets"][j]:rows["offsets"][j + 1]], rows["dist"][rows["offsets"][j]:rows["offsets"][j + 1]]


def test_row_lengths_with_the_set_as_queries_equal_the_oracles_counts():
    c = ds.cases("mixture")[0]
    rows = rs.radius_rows(c["P"], c["P"], c["eps"])
    assert np.array_equal(rows["lengths"], c["oracle"]["counts"])
    assert np.array_equal(rows["lengths"], oracle.dbscan(c["P"], c["eps"], 1)["counts"])
    P, _, radii = rs.lattice_case()
    for r in radii:
        rows = rs.radius_rows(P, P, r)
        assert np.array_equal(rows["lengths"], oracle.dbscan(P, float(r), 1)["counts"]), float(r)
        assert rows["offsets"][-1] == rows["lengths"].sum() == len(rows["idx"]) == len(rows["dist"])


@pytest.mark.parametrize("name", ["uniform", "duplicates", "scale_up"])
def test_rows_agree_with_a_float64_ball_query_outside_a_band_around_r(name):
    P, Q, r0 = qs.make_set(name)
    Q = Q[:: max(1, len(Q) // 300)]
    r = np.float32(r0 * 3)
    rows = rs.radius_rows(P, Q, r)
    tree = cKDTree(P.astype(np.float64))
    band = 1e-6
    for j in range(len(Q)):
        idx, dist = _rows(rows, j)
        q = Q[j].astype(np.float64)
        surely = set(tree.query_ball_point(q, float(r) * (1 - band)))
        maybe = set(tree.query_ball_point(q, float(r) * (1 + band)))
        got = set(idx.tolist())
        assert surely <= got <= maybe, (name, j)
        assert len(got) == len(idx), "no point twice"
        d64 = np.sqrt(((P[idx].astype(np.float64) - q) ** 2).sum(axis=1))
        assert np.allclose(dist, d64, rtol=1e-6, atol=0)
        assert (np.diff(dist) >= 0).all() and (dist <= r).all()
        tied = np.flatnonzero(np.diff(dist.view(np.int32)) == 0)
        assert (idx[tied] < idx[tied + 1]).all(), "ties in index order"


def test_the_lattice_case_reaches_the_boundary():
    P, Q, (r, below, diag) = rs.lattice_case()
    at, under = rs.radius_rows(P, Q, r), rs.radius_rows(P, Q, below)
    on_boundary = int((at["dist"] == r).sum())
    print("lattice: %d entries at distance exactly r, %d rows with one" % (on_boundary, int((at["lengths"] != under["lengths"]).sum())))
    assert on_boundary >= 500, "members at distance exactly r"
    assert (under["dist"] < r).all() and under["offsets"][-1] == at["offsets"][-1] - on_boundary
    centres = rs.radius_rows(P, Q[200:400], diag)  # the cell centres: their cell's corners at half the diagonal
    assert centres["lengths"].max() <= 8 and (centres["dist"] == diag).sum() >= 200, "the corners lie at exactly half the diagonal"


def test_the_chunk_case_has_every_wanted_length():
    P, Q, picks = rs.chunk_case()
    assert [L for L, _, _ in picks] == list(rs.CHUNK_LENGTHS)
    for L, j, r in picks:
        rows = rs.radius_rows(P, Q[j:j + 1], r)
        assert rows["lengths"][0] == L, (L, j, float(r))


def test_nan_rows_and_nan_points():
    c = ds.cases("nan")[0]
    rows = rs.radius_rows(c["P"], c["Q"], c["eps"])
    assert np.array_equal(rows["lengths"], c["counts"])
    nan_q = np.isnan(c["Q"]).any(axis=1)
    assert nan_q.sum() == 5 and (rows["lengths"][nan_q] == 0).all()
    nan_p = np.flatnonzero(np.isnan(c["P"]).any(axis=1))
    assert len(nan_p) == 7 and not np.isin(rows["idx"], nan_p).any()


def test_ids_name_the_entries():
    P, Q, r0 = qs.make_set("tiny")
    ids = np.int64([900, 7, 55, 123456, 8])
    plain, named = rs.radius_rows(P, Q, 0.8), rs.radius_rows(P, Q, 0.8, ids=ids)
    assert plain["lengths"].max() >= 2 and np.array_equal(plain["offsets"], named["offsets"])
    for j in range(len(Q)):
        assert np.array_equal(np.sort(ids[_rows(plain, j)[0]]), np.sort(_rows(named, j)[0]))
    assert np.array_equal(plain["dist"].view(np.int32), named["dist"].view(np.int32))
