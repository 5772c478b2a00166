"""The packet kernel's round structure (trueknn_team.hip): one SELECT pass per gather -- the queries that finish inside the
step and those that speculate at the extension level side by side --, the `reuse` turn for the queries left over, and the
visit of a query's own block at the edges of the tree.  Every solve is compared bit for bit with the CPU checker."""
import functools

import numpy as np
import pytest
from scipy.spatial import cKDTree

import oracle
from owlraytracing_amd import _lib, datasets

pytestmark = pytest.mark.gpu

N0, SEED0 = 20_000, 20251


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _first_set():
    xyz = datasets.uniform3d(N0, seed=SEED0)
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def _first_ref(k):
    """the checker's solve of the first set at the benchmark's start radius (shared, never written to)"""
    return oracle.trueknn(_first_set(), k, datasets.start_radius(N0, k))


def cpu_levels(xyz, k, r0, levels=8, radii=None):
    """The level at which every query finishes (-1: none of the first ``levels``), without a solve: the Chebyshev distance
    of the k-th other point against r0 * 2^t.  The closed-box test of the reference (deviceCode.cu:38-56) rounds c - r and
    c + r to fp32, so that comparison decides unless the distance lies within 2^-22 (|q| + 2 r) of the radius, four times
    what the two roundings can move a face of the box by; the handful of queries in that band count their box literally."""
    xyz = np.asarray(xyz, np.float32)
    p = xyz.astype(np.float64)
    ok = ~np.isnan(p).any(axis=1)
    d = np.full(len(p), np.inf)
    d[ok] = cKDTree(p[ok]).query(p[ok], k=[k + 1], p=np.inf)[0][:, 0]  # (the query itself is the nearest)
    out = np.full(len(p), -1, np.int32)
    r = np.full(len(p), np.float32(r0), np.float32) if radii is None else np.asarray(radii, np.float32).copy()
    scale = np.abs(np.nan_to_num(p)).max(axis=1)
    for t in range(levels):
        r64 = r.astype(np.float64)
        done = d <= r64
        for q in np.flatnonzero(np.abs(d - r64) <= 2.0 ** -22 * (scale + 2 * r64)):
            lo, hi = xyz - r[q], xyz + r[q]  # (fp32)
            done[q] = int(np.all((np.minimum(lo, hi) <= xyz[q]) & (xyz[q] <= np.maximum(lo, hi)), axis=1).sum()) - 1 >= k
        out[(out < 0) & done] = t
        r = r * np.float32(2)
    return out


@pytest.fixture(scope="module")
def first_engine():
    from owlraytracing_amd.trueknn import TrueKNN
    eng = TrueKNN()
    eng.build(_first_set())
    yield eng
    eng.close()


def _engine():
    from owlraytracing_amd.trueknn import TrueKNN
    return TrueKNN()


def _assert_solve(r, ref, rows=None, ids=None):
    rows = slice(None) if rows is None else rows
    want_idx = ref["idx"][rows] if ids is None else ids[ref["idx"][rows]]
    assert np.array_equal(_np(r["idx"])[rows], want_idx)
    assert np.array_equal(_np(r["dist"])[rows].view(np.int32), ref["dist"][rows].view(np.int32))
    assert np.array_equal(_np(r["intersections"])[rows], ref["intersections"][rows])


@pytest.mark.parametrize("k", [10, 16, 32, 40, 64])
def test_benchmark_schedule_in_small(first_engine, k):
    """One, two, three and four list registers per lane, a full list at k = 16, 32 and 64: the first gather serves levels 0
    and 1 and lists level 2, as on the benchmark's 10 M points."""
    r0 = datasets.start_radius(N0, k)
    ref = _first_ref(k)
    r = first_engine.solve(k, r0, kernel=_lib.KERNEL_TEAM, want_levels=True)
    _assert_solve(r, ref)
    assert r["info"]["rounds"] == ref["rounds"]
    assert r["info"]["total_intersections"] == int(ref["intersections"].sum())
    assert r["info"]["unfinished"] == 0
    want = cpu_levels(_first_set(), k, r0)
    assert np.array_equal(_np(r["levels"]), want)
    if k == 10:
        # the merged pass really mixes both kinds: queries that finish at level 1 and queries that go on to level 2
        share = float((want == 1).mean())
        print("k = 10: %.3f of the queries finish at level 1, %.3f at level 2" % (share, float((want == 2).mean())))
        assert 0.25 <= share <= 0.75
        assert 0.25 <= float((_np(r["levels"]) == 1).mean()) <= 0.75


def three_kinds(cells=11, seed=5):
    """At most 512 points in cells of a coarse grid (pitch 1).  With R = 0.05 the outer radius of the first step (levels 0 and
    1, r0 = R / 2; level 2, radius 2 R, is its extension) a cell holds, around its corner c:
      a blob of 40 points within 0.3 R of c                       -- finish inside the step
      a clump of 4 at c + 1.5 R (even cells) / c + 3 R (odd) in x -- 3 others at level 1: speculate at level 2; the blob is in
                                                                     reach there (even: finish at level 2) or not (odd: level 3)
      a point at c + 1.6 R in y                                   -- nobody at level 1: no speculation, the turn for the queries
                                                                     left over counts the blob for it at level 2
      a point at c + 6 R in z                                     -- nobody up to level 3"""
    rng = np.random.default_rng(seed)
    R = np.float32(0.05)
    pts = []
    for c in range(cells):
        corner = np.float32([c % 3, (c // 3) % 2, c // 6]) + np.float32(0.25)
        pts.append(corner + rng.uniform(-0.3, 0.3, (40, 3)).astype(np.float32) * R)
        clump = corner + np.float32([1.5 if c % 2 == 0 else 3.0, 0, 0]) * R
        pts.append(clump + rng.uniform(-0.05, 0.05, (4, 3)).astype(np.float32) * R)
        pts.append((corner + np.float32([0, 1.6, 0]) * R)[None])
        pts.append((corner + np.float32([0, 0, 6.0]) * R)[None])
    xyz = np.ascontiguousarray(np.concatenate(pts), np.float32)
    kinds = np.tile(np.repeat(np.arange(4), [40, 4, 1, 1]), cells)
    odd = (np.repeat(np.arange(cells), 46) % 2) == 1
    return xyz, float(R) / 2, kinds, odd


def test_three_kinds_of_queries_in_one_packet():
    xyz, r0, kinds, odd = three_kinds()
    assert len(xyz) <= 512
    k = 10
    ref = oracle.trueknn(xyz, k, r0)
    want = cpu_levels(xyz, k, r0)
    # the set is what it is meant to be: inside the step | at the extension level, by speculation and by the count of the
    # turn for the rest | beyond it
    assert (want[kinds == 0] <= 1).all()
    assert (want[(kinds == 1) & ~odd] == 2).all() and (want[(kinds == 1) & odd] == 3).all()
    assert (want[kinds == 2] == 2).all() and (want[kinds == 3] >= 4).all()
    eng = _engine()
    eng.build(xyz)
    r = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, want_levels=True)
    eng.close()
    _assert_solve(r, ref)
    assert r["info"]["rounds"] == ref["rounds"]
    assert r["info"]["total_intersections"] == int(ref["intersections"].sum())
    got = _np(r["levels"])
    assert np.array_equal(got, want)
    assert (got <= 1).any() and (got == 2).any() and (got > 2).any()


@pytest.mark.parametrize("max_rounds", [2, 3])
def test_round_limits(first_engine, max_rounds):
    """max_rounds = 2: the first step (levels 0 and 1) has no extension level; 3: its extension level is the last one allowed.
    A row never depends on other rows, so the checker solves the queries that finish in time under the same limit."""
    k = 10
    r0 = datasets.start_radius(N0, k)
    levels = cpu_levels(_first_set(), k, r0, levels=max_rounds)
    in_time = np.flatnonzero(levels >= 0).astype(np.int32)
    assert 0 < len(in_time) and (len(in_time) < N0) == (max_rounds == 2)  # three rounds are what the set needs
    ref = oracle.trueknn(_first_set(), k, r0, query_ids=in_time, max_rounds=max_rounds)
    r = first_engine.solve(k, r0, kernel=_lib.KERNEL_TEAM, max_rounds=max_rounds, allow_unfinished=True)
    _assert_solve(r, ref, rows=in_time)
    assert np.array_equal(_np(r["levels"]), levels)
    assert r["info"]["unfinished"] == N0 - len(in_time)
    assert r["info"]["rounds"] == max_rounds == ref["rounds"]
    assert r["info"]["total_intersections"] == int(ref["intersections"][in_time].sum())


def test_per_query_start_radii(first_engine):
    """two radius classes, alternating along the curve: every packet holds queries of both schedules"""
    import torch

    k = 10
    r0 = np.float32(datasets.start_radius(N0, k))
    order = first_engine.export_tree()["prim_id"]
    radii = np.empty(N0, np.float32)
    radii[order] = np.where(np.arange(N0) % 2 == 0, r0, r0 * np.float32(0.75))
    ref = oracle.trueknn_per_query(_first_set(), k, radii)
    r = first_engine.solve(k, 1.0, start_radii=torch.from_numpy(radii), kernel=_lib.KERNEL_TEAM, want_levels=True)
    _assert_solve(r, ref)
    assert r["info"]["rounds"] == ref["rounds"]
    assert r["info"]["total_intersections"] == int(ref["intersections"].sum())
    assert np.array_equal(_np(r["levels"]), cpu_levels(_first_set(), k, 0.0, radii=radii))


def test_halo_tree():
    """15 000 own and 5 000 halo points of the first set: the own rows are those of a solve over all of them"""
    k = 10
    r0 = datasets.start_radius(N0, k)
    ref = _first_ref(k)
    pick = np.random.default_rng(3).permutation(N0)
    own, rest = np.sort(pick[:15_000]).astype(np.int32), np.sort(pick[15_000:]).astype(np.int32)
    eng = _engine()
    eng.build(_first_set()[own], own)
    eng.set_halo(_first_set()[rest], rest)
    r = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, want_levels=True)
    eng.close()
    assert np.array_equal(_np(r["idx"]), ref["idx"][own])
    assert np.array_equal(_np(r["dist"]).view(np.int32), ref["dist"][own].view(np.int32))
    assert np.array_equal(_np(r["intersections"]), ref["intersections"][own])
    assert r["info"]["total_intersections"] == int(ref["intersections"][own].sum())
    levels = cpu_levels(_first_set(), k, r0)[own]
    assert np.array_equal(_np(r["levels"]), levels)
    assert r["info"]["rounds"] == int(levels.max()) + 1


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 65])
def test_edges_of_the_own_block_address(n, k):
    """the last block of the tree partly filled, exactly filled, one point into the next; the last packet likewise"""
    xyz = datasets.uniform3d(n, seed=100 + n)
    r0 = datasets.start_radius(n, k)
    eng = _engine()
    eng.build(xyz)
    if n <= k:  # nobody ever has k others: the solve stops at the limit with every query unfinished
        r = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, max_rounds=5, allow_unfinished=True)
        eng.close()
        assert r["info"]["unfinished"] == n and (_np(r["levels"]) == -1).all()
        return
    ref = oracle.trueknn(xyz, k, r0)
    r = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, want_levels=True)
    eng.close()
    _assert_solve(r, ref)
    assert r["info"]["rounds"] == ref["rounds"]
    assert r["info"]["total_intersections"] == int(ref["intersections"].sum())
    assert np.array_equal(_np(r["levels"]), cpu_levels(xyz, k, r0, levels=ref["rounds"]))


@pytest.mark.parametrize("k", [1, 10])
def test_nan_rows_have_no_own_block_to_visit(k):
    """three rows with a NaN among 200: nobody's candidates, and as queries they list no block at all"""
    xyz = datasets.uniform3d(200, seed=77)
    bad = np.array([0, 101, 199])
    xyz[bad[0], 2] = np.nan
    xyz[bad[1]] = np.nan
    xyz[bad[2], 0] = np.nan
    good = np.setdiff1d(np.arange(len(xyz)), bad)
    r0 = datasets.start_radius(len(xyz), k)
    ref = oracle.trueknn(xyz[good], k, r0)
    eng = _engine()
    eng.build(xyz)
    r = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, max_rounds=ref["rounds"] + 2, allow_unfinished=True)
    eng.close()
    assert r["info"]["unfinished"] == len(bad)
    assert np.array_equal(_np(r["idx"])[good], good[ref["idx"]])
    assert np.array_equal(_np(r["dist"])[good].view(np.int32), ref["dist"].view(np.int32))
    assert np.array_equal(_np(r["intersections"])[good], ref["intersections"])
    assert r["info"]["total_intersections"] == int(ref["intersections"].sum())
    levels = _np(r["levels"])
    assert (levels[bad] == -1).all() and np.array_equal(levels[good], cpu_levels(xyz[good], k, r0, levels=ref["rounds"]))


def test_counters_do_not_depend_on_where_the_extension_level_is_served(first_engine, monkeypatch):
    """TKNN_TEAM_MERGE=0: the extension level in a turn of its own, as before -- the same rows and the same statistics"""
    k = 10
    r0 = datasets.start_radius(N0, k)
    monkeypatch.setenv("TKNN_TEAM_MERGE", "1")
    a = first_engine.solve(k, r0, kernel=_lib.KERNEL_TEAM, want_levels=True, want_fb=True)
    monkeypatch.setenv("TKNN_TEAM_MERGE", "0")
    b = first_engine.solve(k, r0, kernel=_lib.KERNEL_TEAM, want_levels=True, want_fb=True)
    for name in ("point_tests", "node_tests", "total_active_rounds", "rounds", "total_intersections", "unfinished", "tie_rows"):
        assert a["info"][name] == b["info"][name], name
    for name in ("idx", "dist", "intersections", "levels", "fb"):
        assert np.array_equal(_np(a[name]).view(np.uint8), _np(b[name]).view(np.uint8)), name
    _assert_solve(a, _first_ref(k))
    assert a["info"]["total_active_rounds"] == int((cpu_levels(_first_set(), k, r0) + 1).sum())
