"""What the GPU tests of tknnHaloSelect, tknnHaloSelectFixed, tknnSegmentMin and tknnDbscanAssign expect (tests/halo_spec.py),
checked on the CPU: the cases are what they claim to be -- overlapping boxes, rows for 64 peers at once, closed bounds, NaN rows,
capacities that overflow and that fit exactly, waves that hold three and more segments -- so that the GPU tests cannot pass
vacuously.  Runs without a GPU."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import halo_spec as hs  # noqa: E402
import tile_sets  # noqa: E402


def _all_cases():
    return [hs.selection_case(f, n) for f in hs.FAMILIES for n in hs.SELECT_N]


def test_sizes_ids_and_nan_rows():
    assert max(hs.SELECT_N) <= 20_000 and set(hs.FIXED_N) <= set(hs.SELECT_N)
    for n in hs.SELECT_N:
        P, ids, nan_rows = hs.points(n)
        assert P.shape == (n, 3) and P.dtype == np.float32 and ids.dtype == np.int32
        assert len(np.unique(ids)) == n and ids.min() >= n and ids.min() >= 1_000_000, "ids far outside 0 .. n - 1"
        assert n < 3 or (np.diff(ids) < 0).any() and (np.diff(ids) > 0).any(), "not monotone"
        assert np.array_equal(np.flatnonzero(np.isnan(P).any(axis=1)), nan_rows)
        assert (len(nan_rows) > 0) == (n >= 15)
        assert (np.isnan(P[nan_rows]).sum(axis=1) == 1).all(), "a NaN in ONE coordinate"


def test_every_nan_row_is_selected_nowhere():
    seen = 0
    for c in _all_cases():
        nan_ids = c["ids"][c["nan_rows"]]
        for p in range(c["npeers"]):
            assert not np.isin(nan_ids, c["lists"][p]).any(), (c["name"], p)
        assert not c["boundary"][c["nan_rows"]].any(), c["name"]
        seen += len(nan_ids)
    assert seen > 0


@pytest.mark.parametrize("family", ["everything_max", "everything_inf"])
def test_everything_counts_all_rows_but_the_nan_rows(family):
    for n in hs.SELECT_N:
        c = hs.selection_case(family, n)
        assert c["npeers"] == 3 and (c["counts"] == n - len(c["nan_rows"])).all(), c["name"]
        assert np.array_equal(c["boundary"], ~np.isnan(c["P"]).any(axis=1))
        assert np.isinf(c["boxes"]).all() == (family == "everything_inf") and np.isfinite(c["boxes"]).all() == (family == "everything_max")


def test_overlaps_hold_rows_twice_for_one_peer_and_for_four_peers():
    for n in hs.SELECT_N:
        c = hs.selection_case("overlaps", n)
        hit = hs.inside_boxes(c["P"], c["boxes"])
        per_peer_boxes = np.stack([hit[c["box_peer"] == p].sum(axis=0) for p in range(c["npeers"])])
        assert (per_peer_boxes >= 2).any(), c["name"] + ": no row in two boxes of one peer"
        assert ((per_peer_boxes > 0).sum(axis=0) >= 4).any(), c["name"] + ": no row for four peers"
        # listed once all the same
        for p in range(c["npeers"]):
            assert len(np.unique(c["lists"][p])) == len(c["lists"][p]) == int((per_peer_boxes[p] > 0).sum())
        assert c["counts"][4] == 0


def test_all_peers_cases_reach_every_bit_of_the_mask():
    for n in hs.SELECT_N:
        c = hs.selection_case("peers_all", n)
        assert c["npeers"] == 64 and sorted(c["box_peer"].tolist()) == list(range(64))
        for_all = np.ones(n, bool)
        for p in range(64):
            for_all &= np.isin(c["ids"], c["lists"][p])
        assert for_all[c["centre"]] and for_all.sum() >= 1, c["name"] + ": no row is selected for all 64 peers"
        c = hs.selection_case("peers_apart", n)
        assert c["npeers"] == 64 and set(c["box_peer"].tolist()) == set(hs.PEERS_APART) == {0, 1, 31, 32, 33, 62, 63}
        for p in range(64):
            assert (c["counts"][p] > 0) == (p in hs.PEERS_APART), (c["name"], p)


def test_degenerate_boxes():
    for n in hs.SELECT_N:
        c = hs.selection_case("degenerate", n)
        b = c["boxes"]
        assert np.array_equal(b[0, :3], b[0, 3:]) and np.array_equal(b[0, :3], c["P"][c["centre"]])
        # the closed-bound box selects exactly the row it was built on
        assert c["lists"][0].tolist() == [int(c["ids"][c["centre"]])], c["name"]
        assert np.array_equal(b[1, :3], b[1, 3:]) and c["counts"][1] == 0
        assert (b[2, :3] > b[2, 3:]).sum() == 1 and c["counts"][2] == 0
        assert np.isnan(b[3]).sum() == 1 and np.isnan(b[4]).sum() == 1 and c["counts"][3] == 0
        assert c["counts"][4] >= 1
        # but for the one bad bound, the boxes of peers 2 and 3 would hold every point
        for j in (2, 3, 4):
            mended = b[j].copy()
            mended[:3], mended[3:] = -2, 2
            assert hs.inside_boxes(c["P"], mended[None, :]).sum() == n - len(c["nan_rows"])
        e = hs.selection_case("no_boxes", n)
        assert len(e["boxes"]) == 0 and e["npeers"] == 3 and (e["counts"] == 0).all() and not e["boundary"].any()
        o = hs.selection_case("one_peer", n)
        assert o["npeers"] == 1 and o["counts"][0] >= 1


def test_scattered_and_planar():
    for n in hs.SELECT_N:
        c = hs.selection_case("scattered", n)
        assert len(c["boxes"]) == 40 and c["npeers"] == 5 and c["counts"][2] == 0 and c["counts"].sum() > 0
        if n >= 4095:
            assert 0 < c["boundary"].mean() < 0.5, "the selected rows are a minority"
        p = hs.selection_case("planar", n)
        assert (p["P"][~np.isnan(p["P"][:, 2]), 2] == 0).all() and (p["boxes"][:, [2, 5]] == 0).all() and p["counts"].sum() > 0


def test_capacities_overflow_fit_and_idle():
    """Over the fixed-capacity cases, each relation of capacity and count occurs for some peer: those of a peer that has rows in
    every family, a peer with room and nothing to send in some."""
    cases = hs.fixed_cases()
    assert len(cases) == len(hs.FIXED_FAMILIES) * len(hs.FIXED_N)
    idle = []
    for family in hs.FIXED_FAMILIES:
        seen = set()
        for c, caps in cases:
            if c["family"] != family:
                continue
            cnt = c["counts"]
            assert caps.shape == cnt.shape and caps.dtype == np.int64 and (caps >= 0).all()
            for name, hit in (("cap == 0 < count", (caps == 0) & (cnt > 0)), ("cap == count - 1", (caps == cnt - 1) & (cnt >= 2)),
                              ("cap == count", (caps == cnt) & (cnt > 0)), ("cap == count + 1", (caps == cnt + 1) & (cnt > 0)),
                              ("ample", caps > cnt + 1)):
                if hit.any():
                    seen.add(name)
            if ((caps > 0) & (cnt == 0)).any():
                idle.append(c["name"])
        assert len(seen) == 5, (family, sorted(seen))
    assert idle, "cap > 0 == count: no peer with room and nothing to send"


def _waves(segment):
    return [segment[s:s + 64] for s in range(0, len(segment) - 63, 64)]


def test_multi_segment_layouts_put_three_segments_into_every_wave():
    rng = np.random.default_rng(1)
    for n in hs.SEGMENT_N:
        for lay, least in (("three", 3), ("five", 5), ("sixty_four", 64)):
            seg, m = hs.layout(lay, n, rng)
            assert seg.dtype == np.int32 and len(seg) == n and (seg < m).all()
            for w in _waves(seg):
                assert (w >= 0).all() and len(np.unique(w)) == least >= 3, (lay, n)
        seg, m = hs.layout("two", n, rng)
        for w in _waves(seg):
            assert len(np.unique(w)) == 2
        seg, m = hs.layout("mixed", n, rng)
        mixed = [w for w in _waves(seg) if (w < 0).any() and (w >= 0).any()]
        assert len(mixed) == len(_waves(seg)), "a wave without both -1 lanes and live lanes"
        if n >= 64:
            assert mixed and all(len(np.unique(w[w >= 0])) >= 3 for w in mixed)
        seg, m = hs.layout("none", n, rng)
        assert (seg == -1).all()
        seg, m = hs.layout("runs", n, rng)
        if n >= 255:
            change = np.flatnonzero(np.diff(seg) != 0)
            assert len(change) and np.diff(change).max() <= 400 and (seg >= 0).all() and m == 5000
    for lay, m_want in (("one", 1), ("two", 3), ("five", 70), ("runs", 5000)):
        seg, m = hs.layout(lay, 100_003, rng)
        assert m == m_want
        if m > 1:
            assert len(np.unique(seg)) < m, "some segments are named by no entry"


def test_value_families_and_presets():
    rng = np.random.default_rng(2)
    n = 257
    v = {name: hs.values(name, n, rng) for name in hs.VALUES}
    assert all(a.dtype == np.int64 and a.shape == (n,) for a in v.values())
    assert (v["small"] >= 0).all() and (v["negative"] < 0).all() and len(np.unique(v["equal"])) == 1
    for name, floor in (("above_2_32", 2 ** 32), ("above_2_53", 2 ** 53)):
        assert (v[name] > floor).all() and len(np.unique(v[name])) > 1 and len(np.unique(v[name] >> 3)) == 1
    assert len(np.unique(v["above_2_53"].astype(np.float64))) == 1, "no double tells them apart"
    assert hs.I64_MIN in v["extremes"] and hs.I64_MAX in v["extremes"]
    seg, m = hs.layout("five", n, rng)
    for val in hs.VALUES:
        truth = hs.segment_min(seg, v[val], np.full(m, hs.I64_MAX))
        assert np.array_equal(hs.preset("minimum", seg, v[val], m, rng), truth)
        assert np.array_equal(hs.segment_min(seg, v[val], hs.preset("below", seg, v[val], m, rng)), np.full(m, hs.I64_MIN))
    named = np.unique(seg)
    before = hs.preset("random", seg, v["small"], m, rng)
    after = hs.segment_min(seg, v["small"], before)
    assert (after[named] < before[named]).any() and (after[named] == before[named]).any(), "some entries fall and some stay"


def test_segment_combinations_cover_the_pairs():
    combos = hs.segment_combos()
    assert len(combos) == len(set(combos)) == 72 and 2 * len(combos) + 10 <= 160, "about 150 launches"
    real = [c for c in combos if c[0] >= 63]
    for a, b, na, nb in ((1, 2, hs.LAYOUTS, hs.VALUES), (1, 3, hs.LAYOUTS, hs.PRESETS), (2, 3, hs.VALUES, hs.PRESETS)):
        assert {(c[a], c[b]) for c in real} == {(x, y) for x in na for y in nb}
    assert {(c[0], c[1]) for c in combos} == {(n, lay) for n in hs.SEGMENT_N for lay in hs.LAYOUTS}
    assert {(c[0], c[3]) for c in combos} == {(n, pre) for n in hs.SEGMENT_N for pre in hs.PRESETS}


def test_every_size_has_a_wave_with_three_segments_that_must_fall():
    """At every size from 63 up some listed combination holds, in its last wave of more than two entries (a partial one at 63, 255
    and 100 003), at least three segments whose `out` entry the call must lower: lanes are left over after the two rounds that
    settle a wave's first two segments.  And some combination has nothing to lower at all."""
    for n in hs.SEGMENT_N:
        if n < 63:
            continue
        busy, idle = 0, 0
        for combo in hs.segment_combos():
            if combo[0] != n:
                continue
            c = hs.segment_case(*combo)
            falls = c["want"] < c["out"]
            start = (n - 1) // 64 * 64
            last = c["segment"][start:] if n - start > 2 else c["segment"][start - 64:start]
            live = last[last >= 0]
            busy += len(np.unique(live[falls[live]])) >= 3
            idle += not falls.any() and (c["segment"] >= 0).any()
        assert busy >= 1 and idle >= 1, (n, busy, idle)


def test_segment_min_equals_a_python_loop():
    for n, lay, val, pre in [(65, "five", "negative", "random"), (257, "mixed", "extremes", "max"), (63, "runs", "above_2_53", "random"),
                             (0, "one", "small", "random"), (64, "none", "small", "random")]:
        c = hs.segment_case(n, lay, val, pre)
        want = [int(x) for x in c["out"]]
        for s, x in zip(c["segment"].tolist(), c["value"].tolist()):
            if s >= 0 and x < want[s]:
                want[s] = x
        assert c["want"].dtype == np.int64 and c["want"].tolist() == want, (n, lay, val, pre)
        assert c["want"] is not c["out"]
        assert np.array_equal(hs.segment_min(c["segment"], c["value"], c["want"]), c["want"]), "a second call changes nothing"


@pytest.mark.parametrize("name", ["lattice", "quantised"])
def test_select_agrees_with_the_single_box_layout_of_tile_sets(name):
    xyz, r0 = tile_sets.tie_set(name)
    own, rest = tile_sets.split(xyz)
    lay = tile_sets.phases(xyz, own, rest, r0, 2)
    lists, boundary = hs.select(xyz[own], own, lay["peer_box"][None, :], [1], 2)
    assert boundary.any() and not boundary.all()
    assert np.array_equal(boundary, tile_sets.inside(xyz[own], lay["peer_box"])) and np.array_equal(boundary, lay["boundary"])
    assert len(lists[0]) == 0 and np.array_equal(lists[1], np.sort(own[boundary]))


def test_row_of_id():
    P, ids, _ = hs.points(257)
    rows = hs.row_of_id(ids)
    some = np.int64([5, 0, 256, 5])
    assert np.array_equal(rows(ids[some]), some)
    with pytest.raises(AssertionError):
        rows(np.int32([3]))


@pytest.mark.parametrize("name", hs.ASSIGN_SETS)
def test_assign_cases(name):
    c = hs.assign_case(name)
    n = len(c["P"])
    core, cl, want = c["core"], c["core_label"], c["want"]
    assert n <= 20_000 and cl.dtype == np.int32 and np.array_equal(cl >= 0, core) and (cl[~core] == -1).all()
    ref = c["oracle"]
    if core.any():
        # order-reversing, with gaps, up to 2**31 - 1
        assert cl.max() == hs.TOP_LABEL == 2 ** 31 - 1
        a, b = ref["labels"][core], cl[core].astype(np.int64)
        order = np.argsort(a, kind="stable")
        assert (np.diff(b[order])[np.diff(a[order]) > 0] < -1).all()
        assert len(np.unique(b)) == len(np.unique(a))
    # the same rows are noise as in the oracle's clustering; the labels of border rows are NOT the oracle's renamed: the smallest
    # new label is the largest old one, so they differ where a border point reaches several clusters (`edges`, below)
    assert np.array_equal(want[core], cl[core]) and np.array_equal(want >= 0, ref["labels"] >= 0)
    if name in ("mixture", "slabs", "nan", "edges", "n255", "n256", "n257"):
        border = ~core & (want >= 0)
        assert core.any() and border.any(), "core and border rows"
        assert (want < 0).any() or name == "slabs", "noise rows (the slabs are dense throughout)"
    if name == "nan":
        bad = np.isnan(c["P"]).any(axis=1)
        assert bad.any() and (want[bad] == -1).all()
    if name == "edges":
        import dbscan_query_spec as dq
        border = np.flatnonzero(~core & (want >= 0))
        several = dq.clusters_reached(c["P"], cl, c["eps"], c["P"][border]) > 1
        renamed = hs.remapped(ref["labels"], ref["labels"] >= 0, ref["clusters"])
        assert several.sum() >= 10 and (want[border][several] != renamed[border][several]).any(), \
            "no border row between two clusters: the smallest label is never one of several"
    assert len(np.unique(c["ids"])) == n and c["ids"].min() >= 2_000_000
