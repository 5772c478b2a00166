"""CPU checks of the values tests/test_engine_tiles_gpu.py expects from the engine's tile surface.

The GPU tests take rows from the replay on the whole set G (oracle.trueknn) and per-query levels from oracle.trueknn_numpy
on G.  Here the numpy restatement is run on exactly what the engine is given in each layout -- the tile with its ids, with
or without a halo, capped at the halo's level -- and must come to those values."""
import numpy as np
import pytest

import oracle
import tile_sets
from oracle.trueknn_numpy import trueknn_numpy


def _same_rows(got, ref, rows):
    assert np.array_equal(got["idx"], ref["idx"][rows])
    assert np.array_equal(got["dist"].view(np.int32), ref["dist"][rows].view(np.int32))
    assert np.array_equal(got["intersections"], ref["intersections"][rows])


@pytest.mark.parametrize("name,k", [("cross", 2), ("lattice", 5), ("lattice", 33), ("quantised", 17)])
def test_restatement_with_ids_equals_the_global_replay(name, k):
    """Relabelled tree (a): the tile G[perm] with ids perm.  Tile + halo (c): the tile's points with their global ids and
    the complement behind them, the tile's rows queried.  Both give the replay's rows of those points on G, and the
    levels of trueknn_numpy on G."""
    xyz, r0 = tile_sets.tie_set(name)
    ref = oracle.trueknn(xyz, k, r0)
    lv = trueknn_numpy(xyz, k, r0)["level"]
    perm = tile_sets.relabel(len(xyz))
    got = trueknn_numpy(xyz[perm], k, r0, ids=perm)
    _same_rows(got, ref, perm)
    assert np.array_equal(got["level"], lv[perm])
    own, rest = tile_sets.split(xyz)
    assert len(own) and len(rest) and np.any(np.diff(own) < 0)  # (ids not monotone in the local rows)
    both = np.concatenate([own, rest])
    got = trueknn_numpy(xyz[both], k, r0, ids=both, query_ids=np.arange(len(own)))
    _same_rows({f: got[f][: len(own)] for f in ("idx", "dist", "intersections")}, ref, own)
    assert np.array_equal(got["level"][: len(own)], lv[own])


@pytest.mark.parametrize("name,k", [("cross", 2), ("lattice", 16), ("lattice", 64), ("lattice", 100)])
def test_capped_levels_of_the_phases(name, k):
    """Phases (d) at halo level cap (tile_sets.phase_cap): the interior queries (outside the complement's widened box) on
    the tile alone, the boundary queries on the tile and the halo of phase 2, and all queries on G, each capped at
    cap + 1 rounds, give the levels on G where those are <= cap and -1 exactly where they are above; the finished rows
    are the replay's."""
    xyz, r0 = tile_sets.tie_set(name)
    ref = oracle.trueknn(xyz, k, r0)
    lv = trueknn_numpy(xyz, k, r0)["level"]
    cap = tile_sets.phase_cap(lv)
    own, rest = tile_sets.split(xyz)
    lay = tile_sets.phases(xyz, own, rest, r0, cap)
    boundary, near = lay["boundary"], lay["near"]
    interior = np.nonzero(~boundary)[0]
    lv_own = lv[own]
    assert boundary.any() and (lv_own[interior] <= cap).any()
    assert (lv > cap).any()
    capped = np.where(lv <= cap, lv, -1)
    glob = trueknn_numpy(xyz, k, r0, max_rounds=cap + 1, stop_quietly=True)
    assert np.array_equal(glob["level"], capped)
    # phase 1: the own tree alone
    got = trueknn_numpy(xyz[own], k, r0, query_ids=interior, ids=own, max_rounds=cap + 1, stop_quietly=True)
    assert np.array_equal(got["level"][interior], capped[own[interior]])
    fin = interior[lv_own[interior] <= cap]
    _same_rows({f: got[f][fin] for f in ("idx", "dist", "intersections")}, ref, own[fin])
    # phase 2: own + the complement's points in the tile's widened box
    both = np.concatenate([own, near])
    queries = np.nonzero(boundary)[0]
    got = trueknn_numpy(xyz[both], k, r0, query_ids=queries, ids=both, max_rounds=cap + 1, stop_quietly=True)
    assert np.array_equal(got["level"][queries], capped[own[queries]])
    fin = queries[lv_own[queries] <= cap]
    _same_rows({f: got[f][fin] for f in ("idx", "dist", "intersections")}, ref, own[fin])


@pytest.mark.parametrize("k", [2, 3])
def test_relabelled_cross_round_set_needs_the_level_key(k):
    """The rows of case (a) on the cross-round set whose (distance, id) order is not the replay's: the tie pass must take
    the level at which each neighbour became a candidate for them.  Ids are positions in G, so relabelling moves these
    rows to other local rows and leaves their count as it is.  At k = 2 each of them also ties with the best candidate
    left out of the row, which the tie pass always walks for; at k = 3 none does, so the pass first looks at the written
    row -- the look an id-built tree must not take through the table of rows."""
    xyz, r0 = tile_sets.tie_set("cross")
    ref = oracle.trueknn(xyz, k, r0)
    perm = tile_sets.relabel(len(xyz))
    need = tile_sets.tie_order_needs_level(ref["idx"][perm], ref["dist"][perm])
    assert need.sum() >= 50
    # the ids of those rows, read as rows of the relabelled tree, are other points
    ids = ref["idx"][perm][need]
    assert (ids < len(xyz)).all() and not np.array_equal(xyz[perm][ids], xyz[ids])
    # the nearest point outside the row, by brute force: tied with the row's last entry at k = 2, farther at k = 3
    _, bd = oracle.bruteforce_knn(xyz, k + 1)
    beyond, last = bd[perm][need, k], ref["dist"][perm][need, k - 1]
    assert (beyond == last).all() if k == 2 else (beyond > last).all()


def test_halo_boxes_contain_every_candidate_up_to_the_cap():
    """The boxes of the phase layout are rounded outward: every point of the complement within the halo radius of a tile
    point (closed fp32 box test, the candidate test of the last capped level) is in the phase-2 halo, and no such pair
    has its tile point outside the peer box."""
    xyz, r0 = tile_sets.tie_set("lattice")
    own, rest = tile_sets.split(xyz)
    for cap in (1, 2, 3):  # (level 0, radius 0.02, reaches no other point of the 1/32 lattice)
        lay = tile_sets.phases(xyz, own, rest, r0, cap)
        r = lay["radius"]
        c = xyz[rest]
        lo, hi = (c - r).astype(np.float32), (c + r).astype(np.float32)
        q = xyz[own]
        reach = np.all((lo[None] <= q[:, None]) & (q[:, None] <= hi[None]), axis=2)  # (tile, complement)
        assert reach.any()
        assert np.isin(rest[reach.any(axis=0)], lay["near"]).all()
        assert lay["boundary"][reach.any(axis=1)].all()


@pytest.mark.parametrize("k", [5, 17, 50, 64])
def test_clustered_set_needs_levels_and_carries_ties(k):
    """The clustered set the GPU tests hand over to the team walk: several levels, exact-distance ties in the rows of
    both sides of the split, neither side empty."""
    xyz, r0 = tile_sets.clustered()
    own, rest = tile_sets.split(xyz)
    assert len(own) > 0 and len(rest) > 0 and len(own) + len(rest) == len(xyz)
    ref = oracle.trueknn(xyz, k, r0)
    assert ref["rounds"] >= 3
    for side in (own, rest):
        d = ref["dist"][side]
        assert (d[:, 1:] == d[:, :-1]).any()
