"""TrueKNN.radius_query (tknnRadiusQuery: the points of the built set within a radius of points that are not in it, as CSR
rows) against tests/radius_spec.py on a GPU: every row of every set, bit for bit (sort = 1).

| case       | P                                        | Q, r                                                                     |
|------------|------------------------------------------|--------------------------------------------------------------------------|
| sets       | eight sets of query_spec.make_set        | theirs, r = r0 x 1 and x 3 (duplicates: ties; uniform: 500 outside)      |
| lattice    | spacing 1/32                             | nodes, centres, midpoints; r = 1/32 exactly, the float below, sqrt(3)/64 |
| whole set  | 777 uniform                              | r = 4: every row is the whole set (boxes inside the sphere)              |
| chunks     | 4 096 uniform                            | radii that give one query 0, 1, 15, 16, 17, 63, 64, 65 entries           |
| m edges    | 2 000 uniform                            | m = 0, 1, 3, 4, 5, 63, 64, 65, 257                                       |
| nan        | 1 000 uniform, 7 with a NaN coordinate   | uniform, 5 with a NaN coordinate, copies                                 |
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import dbscan_query_spec as ds  # noqa: E402
import query_spec as qs  # noqa: E402
import radius_spec as rs  # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = -1, -3, -5


def _engine(P, ids=None):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(P, ids=ids)
    return eng


def _same(got, want, what):
    """The engine's CSR rows (tensors or arrays) equal the spec's: offsets, indices, and the distances' bits."""
    off, idx, dist = (np.asarray(got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]) for k in ("offsets", "idx", "dist"))
    assert off.dtype == np.int64 and idx.dtype == np.int32 and dist.dtype == np.float32
    bad = np.flatnonzero(np.diff(off) != want["lengths"])
    assert not len(bad), "%s: %d of %d rows differ in length (first: row %d, %d for %d)" % (
        what, len(bad), len(want["lengths"]), bad[0], np.diff(off)[bad[0]], want["lengths"][bad[0]])
    assert np.array_equal(off, want["offsets"]), what
    bad = np.flatnonzero(dist.view(np.int32) != want["dist"].view(np.int32))
    assert not len(bad), "%s: %d of %d distances differ (first: entry %d)" % (what, len(bad), len(dist), bad[0])
    bad = np.flatnonzero(idx != want["idx"])
    assert not len(bad), "%s: %d of %d indices differ (first: entry %d, %d for %d)" % (what, len(bad), len(idx), bad[0], idx[bad[0]], want["idx"][bad[0]])


def _set_rows(name, factor):
    P, Q, r0 = qs.make_set(name)
    r = np.float32(np.float32(r0) * np.float32(factor))
    return P, Q, r, rs.rows_of(("set", name, factor), lambda: rs.radius_rows(P, Q, r))


def _lattice_rows(t):
    P, Q, radii = rs.lattice_case()
    return P, Q, radii[t], rs.rows_of(("lattice", t), lambda: rs.radius_rows(P, Q, radii[t]))


@pytest.mark.parametrize("factor", rs.SET_FACTORS)
@pytest.mark.parametrize("name", rs.SET_NAMES)
def test_rows_equal_the_spec(name, factor):
    P, Q, r, want = _set_rows(name, factor)
    eng = _engine(P)
    got = eng.radius_query(Q, r)
    _same(got, want, "%s x%d" % (name, factor))
    info = got["info"]
    assert info["total"] == want["offsets"][-1] and info["max_row"] == want["lengths"].max() and info["mismatched"] == 0
    assert info["point_tests"] >= info["total"] and got["count_info"]["total"] == info["total"]
    if name == "uniform":
        assert (want["lengths"][-qs.N_WIDE:] == 0).any(), "queries outside the tree's bounds: empty rows"
    if name == "duplicates" and factor == 3:
        assert (np.diff(want["dist"].view(np.int32))[np.diff(want["idx"]) > 0] == 0).sum() > 100, "distance ties, ordered by index"
    eng.close()


@pytest.mark.parametrize("t", [0, 1, 2])
def test_lattice_boundary(t):
    """r = 1/32 exactly: neighbours at distance exactly r are in; the float below: they are out; sqrt(3)/64: the cell centres."""
    P, Q, r, want = _lattice_rows(t)
    eng = _engine(P)
    _same(eng.radius_query(Q, r), want, "lattice r=%r" % float(r))
    if t == 0:
        assert (want["dist"] == r).sum() >= 500
    if t == 1:
        assert (want["dist"] < rs.LATTICE_STEP).all()
    eng.close()


def test_whole_set_rows():
    """Every row is the whole set: the boxes lie inside the sphere, the count is arithmetic and the fill streams the slots."""
    from owlraytracing_amd import datasets

    P = datasets.uniform3d(777, seed=53)
    Q = np.concatenate([P[:40], np.random.default_rng(54).random((25, 3), dtype=np.float32)])
    want = rs.radius_rows(P, Q, 4.0)
    assert (want["lengths"] == 777).all()
    eng = _engine(P)
    got = eng.radius_query(Q, 4.0)
    _same(got, want, "whole set")
    assert got["count_info"]["point_tests"] < got["info"]["point_tests"], "the count pass adds boxes inside the sphere without reading them"
    # a larger tree: boxes above the leaf level lie inside, too
    P = datasets.uniform3d(40000, seed=55)
    Q = Q[:6]
    want = rs.radius_rows(P, Q, 4.0)
    eng.build(P)
    got = eng.radius_query(Q, 4.0)
    _same(got, want, "whole set, 40 000")
    assert got["count_info"]["point_tests"] < 6 * 40000 // 10
    eng.close()


def test_chunk_edges():
    P, Q, picks = rs.chunk_case()
    eng = _engine(P)
    seen = []
    for L, j, r in picks:
        want = rs.radius_rows(P, Q, r)
        assert want["lengths"][j] == L
        seen.append(int(want["lengths"][j]))
        _same(eng.radius_query(Q, r), want, "chunks L=%d" % L)
    assert seen == list(rs.CHUNK_LENGTHS)
    eng.close()


def test_query_count_edges():
    from owlraytracing_amd import datasets

    P = datasets.uniform3d(2000, seed=56)
    rng = np.random.default_rng(57)
    eng = _engine(P)
    for m in (1, 3, 4, 5, 63, 64, 65, 257):
        Q = rng.random((m, 3), dtype=np.float32)
        _same(eng.radius_query(Q, 0.11), rs.radius_rows(P, Q, 0.11), "m=%d" % m)
    empty = eng.radius_query(np.zeros((0, 3), np.float32), 0.11)
    assert empty["offsets"].cpu().tolist() == [0] and empty["idx"].shape == (0,) and empty["dist"].shape == (0,)
    assert empty["info"]["total"] == 0 and empty["info"]["solve_ms"] == 0
    eng.close()


def test_nan_queries_and_nan_points():
    c = ds.cases("nan")[0]
    want = rs.radius_rows(c["P"], c["Q"], c["eps"])
    nan_q = np.isnan(c["Q"]).any(axis=1)
    assert nan_q.sum() == 5 and (want["lengths"][nan_q] == 0).all()
    eng = _engine(c["P"])
    got = eng.radius_query(c["Q"], c["eps"])
    _same(got, want, "nan")
    assert not np.isin(got["idx"].cpu().numpy(), np.flatnonzero(np.isnan(c["P"]).any(axis=1))).any()
    _same(eng.radius_query(c["Q"], 3.0), rs.radius_rows(c["P"], c["Q"], 3.0), "nan, everything in reach")
    eng.close()


@pytest.mark.parametrize("kind", ["permuted", "above_n"])
def test_ids(kind):
    import torch

    P, Q, r0 = qs.make_set("duplicates")
    Q = Q[::3]
    n = len(P)
    perm = np.random.default_rng(58).permutation(n).astype(np.int32)
    ids = perm if kind == "permuted" else (perm * 3 + 1_000_000).astype(np.int32)
    eng = _engine(torch.from_numpy(np.array(P)).cuda(), torch.from_numpy(ids.copy()).cuda())
    r = np.float32(r0 * 2)
    _same(eng.radius_query(Q, r), rs.radius_rows(P, Q, r, ids=ids), "ids " + kind)
    eng.close()


def test_agrees_with_the_dbscan_calls():
    c = ds.cases("mixture")[0]
    eng = _engine(c["P"])
    got = eng.radius_query(c["Q"], c["eps"])
    lengths = np.diff(got["offsets"].cpu().numpy())
    counted = eng.dbscan_query(c["Q"], c["eps"], c["core_label"], want_counts=True)["counts"].cpu().numpy()
    assert np.array_equal(lengths, counted) and np.array_equal(lengths, c["counts"])
    own = np.diff(eng.radius_query(c["P"], c["eps"])["offsets"].cpu().numpy())
    assert np.array_equal(own, eng.dbscan(c["eps"], 1, want_counts=True)["counts"].cpu().numpy())
    eng.close()


def test_unsorted_rows_hold_the_same_pairs():
    P, Q, r, want = _set_rows("clustered", 3)
    eng = _engine(P)
    got = eng.radius_query(Q, r, sort=False)
    off, idx, dist = got["offsets"].cpu().numpy(), got["idx"].cpu().numpy(), got["dist"].cpu().numpy()
    assert np.array_equal(off, want["offsets"])
    # each row as a sorted set of (dist, idx) pairs: one lexsort over (row, dist, idx)
    row = np.repeat(np.arange(len(Q)), np.diff(off))
    o = np.lexsort((idx, dist, row))
    assert np.array_equal(idx[o], want["idx"]) and np.array_equal(dist[o].view(np.int32), want["dist"].view(np.int32))
    assert got["info"]["sort_ms"] == 0
    only_idx = eng.radius_query(Q, r, want_dist=False)
    assert "dist" not in only_idx and np.array_equal(only_idx["idx"].cpu().numpy(), want["idx"])
    eng.close()


_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import query_spec as qs, radius_spec as rs
from owlraytracing_amd.trueknn import TrueKNN
out = {}
P, Q, r0 = qs.make_set("uniform")
LP, LQ, radii = rs.lattice_case()
eng = TrueKNN(device=0)
for name, P, Q, r in (("uniform", P, Q, np.float32(np.float32(r0) * np.float32(3))), ("lattice", LP, LQ, radii[0])):
    eng.build(P)
    got = eng.radius_query(Q, r)
    assert got["info"]["node_tests"] > 0
    for k in ("offsets", "idx", "dist"):
        out[name + "/" + k] = got[k].cpu().numpy()
eng.close()
np.savez(sys.argv[1], **out)
print("fallback ok")
"""


def test_forced_fallback_in_a_child_process(tmp_path):
    """TKNN_RADIUS_FORCE_FALLBACK=1: the walk leaves every query to the one-query-per-lane kernel, as it does on stack exhaustion."""
    env = dict(os.environ, TKNN_RADIUS_FORCE_FALLBACK="1")
    p = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests")), str(tmp_path / "rows.npz")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "fallback ok" in p.stdout, p.stdout + p.stderr
    got = np.load(tmp_path / "rows.npz")
    _same({k: got["uniform/" + k] for k in ("offsets", "idx", "dist")}, _set_rows("uniform", 3)[3], "fallback, uniform")
    _same({k: got["lattice/" + k] for k in ("offsets", "idx", "dist")}, _lattice_rows(0)[3], "fallback, lattice")


def test_error_codes_in_order_and_bounded_writes():
    import torch

    from owlraytracing_amd import _lib
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _lib.load()
    P, Q, r, want = _lattice_rows(0)
    total, m = int(want["offsets"][-1]), len(Q)
    eng = TrueKNN(device=0)
    dev = eng.device
    q = torch.from_numpy(np.array(Q)).to(dev)
    guard = 4096
    offsets = torch.full((m + 1,), -7, dtype=torch.int64, device=dev)
    idx = torch.full((total + guard,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((total + guard,), -7.0, dtype=torch.float32, device=dev)
    info = _lib.RadiusInfo()

    def call(handle=None, options=True, count=False, **kw):
        o = _lib.RadiusOptions()
        o.d_queries, o.m, o.radius, o.sort, o.d_offsets = q.data_ptr(), m, float(r), 1, offsets.data_ptr()
        if not count:
            o.d_idx, o.d_dist, o.capacity = idx.data_ptr(), dist.data_ptr(), total
        for name, v in kw.items():
            setattr(o, name, v)
        return lib.tknnRadiusQuery(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)

    def untouched():
        return bool((idx == -7).all()) and bool((dist == -7.0).all())

    assert call(handle=ctypes.c_void_p()) == ARG and call(options=False) == ARG
    assert call(d_offsets=None) == ARG and call(d_queries=None) == ARG
    assert call(count=True) == STATE and call(radius=0.0) == STATE and call(m=-1) == STATE  # not built: before any look at the values
    assert call(d_offsets=None, radius=0.0) == ARG  # a missing pointer: before the state
    eng.build(P)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(count=True, radius=bad) == ARG
    assert call(m=-1) == ARG and call(m=2**31 - 1) == ARG and call(d_idx=None) == ARG and call(capacity=-1) == ARG
    assert (offsets == -7).all() and untouched(), "a refused call writes nothing"
    info.node_tests = 99
    assert call(count=True, m=0, d_queries=None) == 0 and info.node_tests == 0 and info.total == 0 and info.solve_ms == 0
    assert offsets[0].item() == 0 and (offsets[1:] == -7).all()
    # the count pass, then a capacity below the total: refused before anything is launched
    assert call(count=True) == 0 and info.total == total and info.max_row == want["lengths"].max() and info.mismatched == 0
    assert np.array_equal(offsets.cpu().numpy(), want["offsets"])
    assert call(capacity=total - 1) == ARG and "capacity" in lib.tknnLastError().decode() and untouched()
    # tknnSolve rows before and after a radius call are identical
    before = eng.solve(5, 0.02)
    assert call() == 0 and info.total == total and info.mismatched == 0 and info.point_tests >= total
    assert info.solve_ms >= info.walk_ms > 0 and info.sort_ms > 0
    after = eng.solve(5, 0.02)
    for k in ("idx", "dist", "intersections"):
        assert torch.equal(before[k], after[k]), k
    _same({"offsets": offsets, "idx": idx[:total], "dist": dist[:total]}, want, "through ctypes")
    assert (idx[total:] == -7).all() and (dist[total:] == -7.0).all()
    # offsets of another radius: every write stays inside its segment and below the capacity, the call says what happened
    for sort in (1, 0):
        idx.fill_(-7), dist.fill_(-7.0)
        wide = np.float32(r * 2)
        assert call(radius=float(wide), sort=sort) == STATE and info.mismatched > 0, sort
        assert "differ in length" in lib.tknnLastError().decode()
        assert (idx[total:] == -7).all() and (dist[total:] == -7.0).all(), "the guard zone behind the capacity"
        if sort == 0:  # what was written: neighbours of the row's query at the wider radius, inside the row's segment
            wide_rows = rs.radius_rows(P, Q, wide)
            got = idx[:total].cpu().numpy()
            for j in range(0, m, 7):
                seg = got[want["offsets"][j]:want["offsets"][j + 1]]
                assert np.isin(seg[seg != -7], wide_rows["idx"][wide_rows["offsets"][j]:wide_rows["offsets"][j + 1]]).all(), j
    narrow = np.nextafter(r, np.float32(0))
    assert call(radius=float(narrow)) == STATE and info.mismatched == int((_lattice_rows(1)[3]["lengths"] != want["lengths"]).sum())
    # offsets that describe no segments at all: nothing is written
    idx.fill_(-7), dist.fill_(-7.0)
    offsets.copy_(-1 - torch.arange(m + 1, dtype=torch.int64, device=dev))
    offsets[m] = total
    assert call(sort=0) == STATE and info.mismatched == m and untouched()
    assert call(sort=1) == STATE and info.mismatched == m and untouched()
    # a halo tree is ignored
    offsets.copy_(torch.from_numpy(want["offsets"]).to(dev))
    eng.set_halo(P[:50], np.arange(50, dtype=np.int32) + 5000)
    assert call() == 0
    _same({"offsets": offsets, "idx": idx[:total], "dist": dist[:total]}, want, "with a halo tree set")
    eng.close()


def test_too_many_neighbours_for_one_call():
    """2^31 or more entries: the count pass says so (its boxes inside the sphere are added, not walked: the call is cheap)."""
    import torch

    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _lib.load()
    eng = TrueKNN(device=0)
    eng.build(datasets.uniform3d(40000, seed=59))
    m = 60000
    q = torch.rand((m, 3), dtype=torch.float32, device=eng.device)
    offsets = torch.empty((m + 1,), dtype=torch.int64, device=eng.device)
    o, info = _lib.RadiusOptions(), _lib.RadiusInfo()
    o.d_queries, o.m, o.radius, o.sort, o.d_offsets = q.data_ptr(), m, 4.0, 1, offsets.data_ptr()
    assert lib.tknnRadiusQuery(eng._h, ctypes.byref(o), ctypes.byref(info), None) == UNSUPPORTED
    assert "split the queries" in lib.tknnLastError().decode() and info.total == 40000 * m and info.max_row == 40000
    assert offsets[m].item() == 40000 * m
    eng.close()


def test_python_front_end():
    import torch

    from owlraytracing_amd.trueknn import radius_query

    P, Q, r, want = _lattice_rows(2)
    res = radius_query(P, Q, r)
    _same(res, want, "one-shot helper")
    assert res["info"]["total"] == want["offsets"][-1] and res["build_info"]["n"] == len(P)
    eng = _engine(P)
    _same(eng.radius_query(torch.from_numpy(np.array(Q)).cuda(), r), want, "a device tensor")
    planar = eng.radius_query(np.array(Q[:10, :2]), 0.1)  # (m, 2): z = 0
    _same(planar, rs.radius_rows(P, np.array(Q[:10, :2]), 0.1), "(m, 2) queries")
    nothing = eng.radius_query(Q[:10] + np.float32(50), r)
    assert nothing["offsets"].cpu().tolist() == [0] * 11 and nothing["idx"].shape == (0,)
    for bad in (Q.astype(np.float64)[:, :1], torch.from_numpy(np.array(Q)), torch.from_numpy(np.array(Q)).cuda().double(),
                torch.from_numpy(np.array(Q)).cuda()[:, :2], torch.from_numpy(np.array(Q)).cuda()[::2]):
        with pytest.raises(ValueError):
            eng.radius_query(bad, r)
    eng.close()
