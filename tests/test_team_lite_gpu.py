"""The packet kernel's light SELECT rounds (team_pass, TKNN_TEAM_LITE): queries that finish inside a step with at most
sixteen others in their box take their short list in list order, every in-box point ungated, and one sort instead of
the gated, ordered SELECT path.  Nothing may change: every case solves with the team kernel twice -- the default and TKNN_TEAM_LITE=0, the usual
path for every round -- and requires idx, dist, intersections and levels to be equal between the two, byte for byte, and
equal to the replay (oracle.trueknn; levels: cpu_levels), and the statistics of the two solves to be equal."""
import functools

import numpy as np
import pytest

import oracle
from owlraytracing_amd import _lib, datasets

from conftest import assert_rows_equal, load_golden
from test_team_rounds_gpu import cpu_levels

pytestmark = pytest.mark.gpu

STATS = ("total_intersections", "point_tests", "rounds", "tie_rows", "tie_rows_left", "unfinished")
FIELDS = ("idx", "dist", "intersections", "levels")
N0, SEED0 = 20_000, 20261


def _np(t):
    return t.cpu().numpy()


def _engine():
    from owlraytracing_amd.trueknn import TrueKNN
    return TrueKNN()


def _solve_both(eng, k, r0, monkeypatch, rows=slice(None), **kw):
    """the default solve, after checking that the solve with TKNN_TEAM_LITE=0 gives the same bytes (in rows `rows`: an
    unfinished query's row is never written) and statistics"""
    got = {}
    for lite in ("0", None):
        for name in ("TKNN_TEAM_LITE", "TKNN_TEAM_COUNT_FLAT", "TKNN_TEAM_EXT", "TKNN_TEAM_MERGE"):
            monkeypatch.delenv(name, raising=False)
        if lite is not None:
            monkeypatch.setenv("TKNN_TEAM_LITE", lite)
        got[lite] = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, want_levels=True, **kw)
    on, off = got[None], got["0"]
    for name in FIELDS:
        assert np.array_equal(_np(on[name])[rows].view(np.uint8), _np(off[name])[rows].view(np.uint8)), name + ": differs from TKNN_TEAM_LITE=0"
    for name in STATS:
        assert on["info"][name] == off["info"][name], name + ": differs from TKNN_TEAM_LITE=0"
    assert on["info"]["kernel_used"] == _lib.KERNEL_TEAM
    return on


def _assert_replay(r, ref, levels, rows=None):
    """rows of a solve against the replay's (rows `rows` of it), index for index"""
    pick = slice(None) if rows is None else rows
    assert_rows_equal(_np(r["idx"]), _np(r["dist"]), ref["idx"][pick], ref["dist"][pick])
    assert np.array_equal(_np(r["intersections"]), ref["intersections"][pick]), "intersection counts differ"
    assert np.array_equal(_np(r["levels"]), levels), "levels differ"
    assert r["info"]["total_intersections"] == int(ref["intersections"][pick].sum())
    assert r["info"]["tie_rows_left"] == 0


def _check_set(xyz, k, r0, monkeypatch):
    xyz = np.ascontiguousarray(xyz, np.float32)
    ref = oracle.trueknn(xyz, k, r0)
    eng = _engine()
    eng.build(xyz)
    try:
        r = _solve_both(eng, k, r0, monkeypatch)
    finally:
        eng.close()
    assert r["info"]["rounds"] == ref["rounds"] and r["info"]["unfinished"] == 0
    _assert_replay(r, ref, cpu_levels(xyz, k, r0, levels=ref["rounds"]))
    return r


# ---- uniform cube -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _uniform():
    xyz = datasets.uniform3d(N0, seed=SEED0)
    xyz.setflags(write=False)
    return xyz


@pytest.fixture(scope="module")
def uniform_engine():
    eng = _engine()
    eng.build(_uniform())
    yield eng
    eng.close()


def _others_where_finished(xyz, k, r0, levels=8):
    """per query: the level it finishes at and how many others its box holds there (Chebyshev distances in fp64: the
    sets of this file keep every distance far from a radius)"""
    from scipy.spatial import cKDTree
    p = np.asarray(xyz, np.float64)
    tree = cKDTree(p)
    level = np.full(len(p), -1)
    others = np.zeros(len(p), np.int64)
    r = float(np.float32(r0))
    for t in range(levels):
        cnt = tree.query_ball_point(p, r, p=np.inf, return_length=True) - 1
        now = (level < 0) & (cnt >= k)
        level[now], others[now] = t, cnt[now]
        r *= 2.0
    return level, others


@pytest.mark.parametrize("k", [1, 5, 10, 15, 16, 17])
def test_uniform(uniform_engine, monkeypatch, k):
    """20 000 uniform points at the standard start radius: light and ordinary queries in every packet.  k = 16 is the
    full-list instantiation (a light query there has exactly sixteen others); k = 17 has two list registers per lane, for
    which the path is off."""
    xyz, r0 = _uniform(), datasets.start_radius(N0, k)
    level, others = _others_where_finished(xyz, k, r0)
    light = (level >= 0) & (others <= 16)
    print("k = %d: %d of %d queries finish with at most 16 others in their box" % (k, light.sum(), len(xyz)))
    if k <= 15:
        assert 0.05 * len(xyz) < light.sum() < len(xyz), "the set does not mix light and ordinary queries"
    ref = oracle.trueknn(xyz, k, r0)
    r = _solve_both(uniform_engine, k, r0, monkeypatch)
    assert r["info"]["rounds"] == ref["rounds"] and r["info"]["unfinished"] == 0
    _assert_replay(r, ref, cpu_levels(xyz, k, r0, levels=ref["rounds"]))


# ---- the 16 / 17 boundary -----------------------------------------------------------------------------------------------
CLUMP_BLOB, CLUMP_GAP = 0.001, 0.015  # a clump: two blobs of side <= CLUMP_BLOB whose corners lie CLUMP_GAP apart


@functools.lru_cache(maxsize=None)
def _clumps():
    """57 clumps of exactly 17 points and 57 of exactly 18 (1 995 points) on a grid of spacing 1.  A clump is two tight blobs
    of 9 + 8 or 9 + 9 points: within 0.01 a point sees its own blob only (8 others at most), within 0.02 its whole clump
    and nothing else."""
    rng = np.random.default_rng(1716)
    pts, size = [], []
    for c in range(114):
        n = 17 if c % 2 == 0 else 18
        centre = np.array([c % 5, (c // 5) % 5, c // 25], np.float64)
        blob = rng.random((n, 3)) * CLUMP_BLOB
        blob[9:] += CLUMP_GAP
        pts.append(centre + blob)
        size += [n] * n
    xyz = np.concatenate(pts).astype(np.float32)
    perm = rng.permutation(len(xyz))
    xyz, size = np.ascontiguousarray(xyz[perm]), np.asarray(size)[perm]
    xyz.setflags(write=False)
    return xyz, size


@pytest.mark.parametrize("k", [10, 16])
@pytest.mark.parametrize("at_level", [0, 1])
def test_clumps_of_17_and_18(monkeypatch, k, at_level):
    """Every query of a clump of 17 finishes with exactly 16 others in its box (light), every query of a clump of 18 with
    17 (not light) -- at level 0 with a start radius of 0.02, at level 1 with 0.01."""
    xyz, size = _clumps()
    r0 = 0.02 if at_level == 0 else 0.01
    level, others = _others_where_finished(xyz, k, r0)
    assert (level == at_level).all(), "the construction is wrong: levels %s" % np.unique(level)
    assert (others[size == 17] == 16).all() and (others[size == 18] == 17).all(), "the construction is wrong"
    assert (size == 17).sum() == 57 * 17 and (size == 18).sum() == 57 * 18
    r = _check_set(xyz, k, r0, monkeypatch)
    assert np.array_equal(_np(r["levels"]), level)


# ---- exact ties in light rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 5, 6, 8])
def test_planar_lattice(monkeypatch, k):
    """64 x 64 lattice in the plane z = 0, spacing 1, start radius 0.6: at level 1 an inner point's box holds its eight
    lattice neighbours at distances 1 and sqrt(2).  k = 5 and 6: a tie across entries k - 1 / k; k = 8: others = k."""
    g = np.arange(64, dtype=np.float32)
    xyz = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    xyz = np.concatenate([xyz, np.zeros((len(xyz), 1), np.float32)], 1)
    level, others = _others_where_finished(xyz, k, 0.6)
    inner = (level == 1) & (others == 8)
    assert inner.sum() == 62 * 62, "the construction is wrong"
    r = _check_set(xyz, k, 0.6, monkeypatch)
    if k in (5, 6):
        assert r["info"]["tie_rows"] > 0


@pytest.mark.parametrize("name", ["crossroundties_n400_k2", "boundaryband_n3640_k7"])
def test_golden_tie_sets(monkeypatch, name):
    g = load_golden(name)
    _check_set(g["xyz"], int(g["k"]), float(g["start_radius"]), monkeypatch)


# ---- a halo tree --------------------------------------------------------------------------------------------------------
def test_halo_tree(monkeypatch):
    """5 000 own and 1 000 halo points (the HALO = true instantiation): the own rows of a solve over all of them"""
    k = 10
    xyz = datasets.uniform3d(6_000, seed=43)
    r0 = datasets.start_radius(len(xyz), k)
    ref = oracle.trueknn(xyz, k, r0)
    pick = np.random.default_rng(44).permutation(len(xyz))
    own, rest = np.sort(pick[:5_000]).astype(np.int32), np.sort(pick[5_000:]).astype(np.int32)
    eng = _engine()
    eng.build(xyz[own], own)
    eng.set_halo(xyz[rest], rest)
    try:
        r = _solve_both(eng, k, r0, monkeypatch)
    finally:
        eng.close()
    levels = cpu_levels(xyz, k, r0)[own]
    _assert_replay(r, ref, levels, rows=own)
    assert r["info"]["rounds"] == int(levels.max()) + 1


# ---- per-query start radii ----------------------------------------------------------------------------------------------
def test_per_query_start_radii(monkeypatch):
    """one-level steps (first_step = 1), every query with a radius schedule of its own"""
    import torch
    k = 10
    xyz = datasets.uniform3d(8_000, seed=45)
    base = np.float32(datasets.start_radius(len(xyz), k))
    radii = np.random.default_rng(46).choice(np.float32([0.5, 1.0, 2.0, 4.0]) * base, len(xyz)).astype(np.float32)
    ref = oracle.trueknn_per_query(xyz, k, radii)
    eng = _engine()
    eng.build(xyz)
    try:
        r = _solve_both(eng, k, 1.0, monkeypatch, start_radii=torch.from_numpy(radii))
    finally:
        eng.close()
    assert r["info"]["rounds"] == ref["rounds"]
    _assert_replay(r, ref, cpu_levels(xyz, k, 0.0, levels=ref["rounds"], radii=radii))


# ---- duplicates and NaN -------------------------------------------------------------------------------------------------
def test_duplicates_and_nan(monkeypatch):
    """5 000 points, 5 % of them exact copies of others (told from the query by id only) and four rows with NaN
    coordinates (sentinel points: nobody's candidates, never finished as queries)"""
    k = 5
    xyz = datasets.uniform3d(5_000, seed=47)
    rng = np.random.default_rng(48)
    dup = rng.choice(len(xyz), 250, replace=False)
    src = rng.choice(np.setdiff1d(np.arange(len(xyz)), dup), 250, replace=False)
    xyz[dup] = xyz[src]
    bad = np.setdiff1d(np.array([7, 1234, 3333, 4999]), np.concatenate([dup, src]))
    assert len(bad) >= 2
    xyz[bad[0], 0] = np.nan
    xyz[bad[1], 2] = np.nan
    xyz[bad[2:]] = np.nan
    good = np.setdiff1d(np.arange(len(xyz)), bad)
    r0 = datasets.start_radius(len(xyz), k)
    ref = oracle.trueknn(xyz[good], k, r0)
    eng = _engine()
    eng.build(xyz)
    try:
        r = _solve_both(eng, k, r0, monkeypatch, rows=good, max_rounds=ref["rounds"] + 2, allow_unfinished=True)
    finally:
        eng.close()
    assert r["info"]["unfinished"] == len(bad)
    idx, dist = _np(r["idx"])[good], _np(r["dist"])[good]
    assert not np.isin(idx, bad).any()
    assert_rows_equal(idx, dist, good[ref["idx"]], ref["dist"])
    assert np.array_equal(_np(r["intersections"])[good], ref["intersections"])
    levels = _np(r["levels"])
    assert np.array_equal(levels[good], cpu_levels(xyz[good], k, r0, levels=ref["rounds"])) and (levels[bad] == -1).all()
