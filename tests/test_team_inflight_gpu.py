"""The packet kernel with a COUNT round's block loads all in flight (team_pass's flat path, TKNN_TEAM_COUNT_FLAT) and the
gather's leaf loops reading one child box ahead (trueknn_team.hip).  Neither may change a bit: every solve goes through the
packet kernel and is compared with the CPU checker -- idx, the bits of dist, intersections, levels, rounds -- and the
settings of the flat path are compared with the ring (setting 0) statistic by statistic."""
import functools

import numpy as np
import pytest

import oracle
from owlraytracing_amd import _lib, datasets

from test_team_rounds_gpu import cpu_levels

pytestmark = pytest.mark.gpu

N0, SEED0, K0 = 20_000, 20260, 10
FACTORS = [0.5, 1.0, 2.0, 4.0]  # of datasets.start_radius: two-level first steps (0.5, 1) and one-level ones (2, 4)
STATS = ("total_intersections", "point_tests", "node_tests", "rounds")


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _uniform():
    xyz = datasets.uniform3d(N0, seed=SEED0)
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def _uniform_ref(k, factor):
    """the checker's solve of the uniform set (shared, never written to)"""
    return oracle.trueknn(_uniform(), k, datasets.start_radius(N0, k) * factor)


def _engine():
    from owlraytracing_amd.trueknn import TrueKNN
    return TrueKNN()


@pytest.fixture(scope="module")
def uniform_engine():
    eng = _engine()
    eng.build(_uniform())
    yield eng
    eng.close()


def _solve(eng, k, r0, monkeypatch, env=None, **kw):
    for name in ("TKNN_TEAM_COUNT_FLAT", "TKNN_TEAM_EXT", "TKNN_TEAM_MERGE"):
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    return eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, want_levels=True, **kw)


def _assert_solve(r, ref, xyz, k, r0):
    assert np.array_equal(_np(r["idx"]), ref["idx"])
    assert np.array_equal(_np(r["dist"]).view(np.int32), ref["dist"].view(np.int32))
    assert np.array_equal(_np(r["intersections"]), ref["intersections"])
    assert r["info"]["rounds"] == ref["rounds"]
    assert r["info"]["total_intersections"] == int(ref["intersections"].sum())
    assert r["info"]["unfinished"] == 0
    assert np.array_equal(_np(r["levels"]), cpu_levels(xyz, k, r0, levels=ref["rounds"]))


def first_step_levels(xyz, k, r0):
    """levels the first gather serves (Engine::first_step_estimate, at most two): the first at which a box is expected to
    hold k / 2 points at the set's mean density"""
    ext = (xyz.max(0) - xyz.min(0)).astype(np.float64)
    density = len(xyz) / float(np.prod(ext[ext > 0]))
    dims = int((ext > 0).sum())
    return 1 if density * (2.0 * r0) ** dims >= 0.5 * k else 2


def longest_lists_of_count_rounds(xyz, order, r):
    """The longest front list of every round of the first step's COUNT pass, modelled on the CPU from the tree's point
    order: blocks of 16 sorted points, a query needs a block if the block's box meets [q - r, q + r], the 64 queries of a
    packet are ordered by list length in buckets of four blocks (build_qlist) and served four to a round."""
    p = xyz[order]
    n = len(p)
    pad = np.full(((n + 15) // 16 * 16 - n, 3), np.nan, np.float32)
    blocks = np.concatenate([p, pad]).reshape(-1, 16, 3)
    blo, bhi = np.nanmin(blocks, 1), np.nanmax(blocks, 1)
    longest = []
    for s in range(0, n, 64):
        q = p[s:s + 64]
        near = np.flatnonzero(np.all((blo <= q.max(0) + r) & (bhi >= q.min(0) - r), axis=1))
        need = np.all((blo[near][None] <= (q + r)[:, None]) & (bhi[near][None] >= (q - r)[:, None]), axis=2).sum(1)
        in_order = need[np.argsort(need >> 2, kind="stable")]
        longest.extend(in_order[i:i + 4].max() for i in range(0, len(in_order), 4))
    return np.asarray(longest)


def test_the_uniform_set_has_rounds_of_every_length(uniform_engine):
    """Precondition of the tests below: over the four start radii the first steps' COUNT rounds have longest lists of at
    most 4, of 5 to 8, of 9 to 12 (one, two and three groups on the flat path) and of more than 12 blocks (the ring)."""
    order = uniform_engine.export_tree()["prim_id"]
    seen = np.zeros(4, np.int64)
    for factor in FACTORS:
        r0 = np.float32(datasets.start_radius(N0, K0) * factor)
        r_out = r0 * np.float32(2 ** (first_step_levels(_uniform(), K0, float(r0)) - 1))
        longest = longest_lists_of_count_rounds(_uniform(), order, r_out)
        kinds = np.bincount(np.digitize(longest, [5, 9, 13]), minlength=4)
        print("start radius x %.1f, step radius %.5f: rounds with a longest list <= 4 / 5-8 / 9-12 / > 12: %s" % (factor, r_out, kinds))
        seen += kinds
    assert (seen > 0).all(), seen


@pytest.mark.parametrize("factor", FACTORS)
def test_uniform_every_setting_equals_the_ring(uniform_engine, monkeypatch, factor):
    """TKNN_TEAM_COUNT_FLAT = 0 (the ring for every round), 4, 8 and the default, then the default against 0 without
    extended gathers (TKNN_TEAM_EXT=0) and with the extension level in a turn of its own (TKNN_TEAM_MERGE=0)"""
    r0 = datasets.start_radius(N0, K0) * factor
    ref = _uniform_ref(K0, factor)
    for other in ({}, {"TKNN_TEAM_EXT": "0"}, {"TKNN_TEAM_MERGE": "0"}):
        ring = _solve(uniform_engine, K0, r0, monkeypatch, dict(other, TKNN_TEAM_COUNT_FLAT="0"))
        _assert_solve(ring, ref, _uniform(), K0, r0)
        for flat in (["4", "8", None] if not other else [None]):
            env = dict(other) if flat is None else dict(other, TKNN_TEAM_COUNT_FLAT=flat)
            r = _solve(uniform_engine, K0, r0, monkeypatch, env)
            _assert_solve(r, ref, _uniform(), K0, r0)
            for name in STATS:
                assert r["info"][name] == ring["info"][name], (env, name)
            for name in ("idx", "dist", "intersections", "levels"):
                assert np.array_equal(_np(r[name]).view(np.uint8), _np(ring[name]).view(np.uint8)), (env, name)


@pytest.mark.parametrize("k", [16, 32, 64])
def test_larger_lists_share_the_count_pass(uniform_engine, monkeypatch, k):
    """two and four list registers per lane, full lists: other instantiations of the kernel, the same COUNT pass"""
    r0 = datasets.start_radius(N0, k)
    _assert_solve(_solve(uniform_engine, k, r0, monkeypatch), _uniform_ref(k, 1.0), _uniform(), k, r0)


def _edge_set(name):
    if name == "duplicates":  # every point six times over: lists of blocks full of one point, ties at distance 0
        xyz = np.repeat(datasets.uniform3d(5_000 // 6 + 1, seed=31), 6, axis=0)[:5_000]
        return np.ascontiguousarray(xyz[np.random.default_rng(32).permutation(len(xyz))]), 0.01
    if name == "planar":  # z = 0: two axes differ
        xyz = datasets.uniform3d(5_000, seed=33)
        xyz[:, 2] = 0.0
        return xyz, 0.25 * (3.0 / 5_000) ** 0.5
    n = int(name)
    return datasets.uniform3d(n, seed=200 + n), datasets.start_radius(n, 3)


@pytest.mark.parametrize("name", ["17", "65", "130", "1000", "duplicates", "planar"])
def test_edges(monkeypatch, name):
    """k = 3.  n = 17: a last block of one point beside NaN padding; 65: a last packet of one query (three teams of its
    rounds without a query); 130: a tree of two packets and a bit; a duplicate-heavy and a planar set"""
    xyz, r0 = _edge_set(name)
    ref = oracle.trueknn(xyz, 3, r0)
    eng = _engine()
    eng.build(xyz)
    ring = _solve(eng, 3, r0, monkeypatch, {"TKNN_TEAM_COUNT_FLAT": "0"})
    r = _solve(eng, 3, r0, monkeypatch)
    eng.close()
    _assert_solve(ring, ref, xyz, 3, r0)
    _assert_solve(r, ref, xyz, 3, r0)
    for stat in STATS:
        assert r["info"][stat] == ring["info"][stat], stat


def test_halo_tree(monkeypatch):
    """5 000 own and 5 000 halo points (the HALO = true instantiation): the own rows of a solve over all of them"""
    k = K0
    xyz = datasets.uniform3d(10_000, seed=41)
    r0 = datasets.start_radius(len(xyz), k)
    ref = oracle.trueknn(xyz, k, r0)
    pick = np.random.default_rng(42).permutation(len(xyz))
    own, rest = np.sort(pick[:5_000]).astype(np.int32), np.sort(pick[5_000:]).astype(np.int32)
    eng = _engine()
    eng.build(xyz[own], own)
    eng.set_halo(xyz[rest], rest)
    ring = _solve(eng, k, r0, monkeypatch, {"TKNN_TEAM_COUNT_FLAT": "0"})
    r = _solve(eng, k, r0, monkeypatch)
    eng.close()
    levels = cpu_levels(xyz, k, r0)[own]
    for got in (ring, r):
        assert np.array_equal(_np(got["idx"]), ref["idx"][own])
        assert np.array_equal(_np(got["dist"]).view(np.int32), ref["dist"][own].view(np.int32))
        assert np.array_equal(_np(got["intersections"]), ref["intersections"][own])
        assert got["info"]["total_intersections"] == int(ref["intersections"][own].sum())
        assert np.array_equal(_np(got["levels"]), levels)
        assert got["info"]["rounds"] == int(levels.max()) + 1
    for stat in STATS:
        assert r["info"][stat] == ring["info"][stat], stat
