"""The packet kernel's PLAIN instantiation (team_kernel<..., PLAIN>, PlainTeamArgs): a solve that writes idx, dist and
intersections and nothing else -- no frame buffer, no per-query start radii, no levels, no phase, no halo tree, no
measurement knob, k <= 16 -- runs a kernel that carries none of that, on an argument block of what is left.  Nothing may
change: every case solves twice on one engine, as it comes and with TKNN_TEAM_PLAIN=0 (the generic instantiation), and
requires idx, dist and intersections of the two solves to be equal byte for byte and equal to the replay (oracle.trueknn).
The engine says which instantiation a solve took (TKNN_VERBOSE), so a case cannot pass without the kernel it is about."""
import functools
import re

import numpy as np
import pytest

import oracle
from owlraytracing_amd import _lib, datasets

import tile_sets
from conftest import assert_rows_equal
from test_team_rounds_gpu import cpu_levels

pytestmark = pytest.mark.gpu

FIELDS = ("idx", "dist", "intersections")
STATS = ("total_intersections", "point_tests", "rounds", "tie_rows", "tie_rows_left", "unfinished")
KNOBS = ("TKNN_TEAM_PLAIN", "TKNN_TEAM_LITE", "TKNN_TEAM_COUNT_FLAT", "TKNN_TEAM_EXT", "TKNN_TEAM_MERGE", "TKNN_TEAM_DIAG")


def _np(t):
    return t.cpu().numpy()


def _engine():
    from owlraytracing_amd.trueknn import TrueKNN
    return TrueKNN()


def _said(capfd):
    """(which instantiations the solves since the last look took, how many queries they handed over)"""
    err = capfd.readouterr().err
    took = re.findall(r"\[team\] packet kernel: the (\w+) instantiation", err)
    handed = sum(int(m) for m in re.findall(r"\[team\] (\d+) of \d+ queries handed over", err))
    return took, handed


def _solve_both(eng, k, r0, monkeypatch, capfd, expect="plain", rows=slice(None), **kw):
    """the solve as it comes, after checking that it took the `expect`ed instantiation and that the solve with
    TKNN_TEAM_PLAIN=0 took the generic one and gives the same bytes (in rows `rows`) and statistics; and how many
    queries the first of them handed over"""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("TKNN_VERBOSE", "1")
    capfd.readouterr()
    on = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, **kw)
    took, handed = _said(capfd)
    assert took == [expect], "the solve took %s" % took
    monkeypatch.setenv("TKNN_TEAM_PLAIN", "0")
    off = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, **kw)
    monkeypatch.delenv("TKNN_TEAM_PLAIN")
    took, handed_off = _said(capfd)
    assert took == ["generic"], "the solve with TKNN_TEAM_PLAIN=0 took %s" % took
    assert handed == handed_off
    for name in FIELDS:
        assert np.array_equal(_np(on[name])[rows].view(np.uint8), _np(off[name])[rows].view(np.uint8)), name + ": differs from TKNN_TEAM_PLAIN=0"
    for name in STATS:
        assert on["info"][name] == off["info"][name], name + ": differs from TKNN_TEAM_PLAIN=0"
    assert on["info"]["kernel_used"] == off["info"]["kernel_used"]
    return on, handed


def _assert_replay(r, ref):
    assert_rows_equal(_np(r["idx"]), _np(r["dist"]), ref["idx"], ref["dist"])
    assert np.array_equal(_np(r["intersections"]), ref["intersections"]), "intersection counts differ"
    assert r["info"]["total_intersections"] == int(ref["intersections"].sum())
    assert r["info"]["rounds"] == ref["rounds"] and r["info"]["unfinished"] == 0 and r["info"]["tie_rows_left"] == 0


def _check_set(xyz, k, r0, monkeypatch, capfd):
    xyz = np.ascontiguousarray(xyz, np.float32)
    ref = oracle.trueknn(xyz, k, r0)
    eng = _engine()
    eng.build(xyz)
    try:
        r, handed = _solve_both(eng, k, r0, monkeypatch, capfd)
    finally:
        eng.close()
    _assert_replay(r, ref)
    return r, ref, handed


@functools.lru_cache(maxsize=None)
def _uniform(n):
    return datasets.uniform3d(n, seed=2027 + n)


# ---- uniform points: a partial last packet, two packets, several chunks of packets -------------------------------------
@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("n", [63, 65, 4097])
def test_uniform(monkeypatch, capfd, n, k):
    """n = 63: one packet, its last lane without a query; 65: a second packet of one query; 4097: 65 packets, dealt to
    the eight XCDs' counters in chunks.  k = 16 fills the list (the FULL instantiation)."""
    _check_set(_uniform(n), k, datasets.start_radius(n, k), monkeypatch, capfd)


def test_many_levels(monkeypatch, capfd):
    """a start radius an eighth of the usual one: turns of the level loop after the extension level, lists kept for the
    next turn (`reuse`), queries served a turn early"""
    n, k = 4097, 10
    xyz, r0 = _uniform(n), datasets.start_radius(n, k) / 8
    level = cpu_levels(xyz, k, r0, levels=12)
    assert np.median(level) >= 3 and level.max() >= 4, "the set is wrong: levels up to %d" % level.max()
    _check_set(xyz, k, r0, monkeypatch, capfd)


# ---- hand-overs: done, isect_sorted and next_level are the plain kernel's stores, too ----------------------------------
def test_clustered_hands_over(monkeypatch, capfd):
    """three tight clusters (sigma 0.004, 1 300 points each) at a start radius of two sigma: a box in a core holds most of
    its cluster, some eighty leaf blocks where a list has 72 slots, so those packets are handed to the tail -- from the
    level and with the count the packet kernel leaves for them; the fringe goes on in the packet kernel"""
    xyz, _ = tile_sets.clustered(4000)
    _, _, handed = _check_set(xyz, 10, 0.008, monkeypatch, capfd)
    assert handed > 0


# ---- exact-distance ties: the tie flags, knn_flag_tie and the tie pass behind the kernel --------------------------------
@pytest.mark.parametrize("k", [10, 16])
def test_lattice(monkeypatch, capfd, k):
    """a full 16^3 lattice of spacing 1/32: every row cuts through a shell of equal distances"""
    g = np.arange(16, dtype=np.float32) / np.float32(32)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    xyz = np.ascontiguousarray(xyz[np.random.default_rng(16).permutation(len(xyz))])
    r, _, _ = _check_set(xyz, k, 0.02, monkeypatch, capfd)
    assert r["info"]["tie_rows"] > 0


# ---- the selection rule -------------------------------------------------------------------------------------------------
def test_one_round_allowed_unfinished_is_generic(monkeypatch, capfd):
    """allow_unfinished with max_rounds = 1 asks for levels: the generic kernel, whose rows at level 0 are the replay's
    and whose other rows are not written.  (Twice the usual start radius: a box is expected to hold k others, so about
    half of the queries finish at level 0.)"""
    n, k = 4097, 10
    xyz, r0 = _uniform(n), 2 * datasets.start_radius(n, k)
    ref = oracle.trueknn(xyz, k, r0)
    level = cpu_levels(xyz, k, r0)
    fin = np.flatnonzero(level == 0)
    assert 0 < len(fin) < n
    eng = _engine()
    eng.build(xyz)
    try:
        r, _ = _solve_both(eng, k, r0, monkeypatch, capfd, expect="generic", rows=fin, max_rounds=1, allow_unfinished=True)
    finally:
        eng.close()
    assert np.array_equal(_np(r["levels"]), np.where(level == 0, 0, -1))
    assert r["info"]["unfinished"] == n - len(fin)
    assert_rows_equal(_np(r["idx"])[fin], _np(r["dist"])[fin], ref["idx"][fin], ref["dist"][fin])
    assert np.array_equal(_np(r["intersections"])[fin], ref["intersections"][fin])


def test_what_the_plain_kernel_lacks_goes_to_the_generic_one(monkeypatch, capfd):
    """a frame buffer, per-query start radii, a phase after a halo selection, a measurement knob: each alone sends the solve
    to the generic kernel, and the rows are what they were"""
    import torch
    n, k = 4097, 10
    xyz, r0 = _uniform(n), datasets.start_radius(n, k)
    ref = oracle.trueknn(xyz, k, r0)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("TKNN_VERBOSE", "1")
    eng = _engine()
    eng.build(xyz)
    try:
        capfd.readouterr()
        # the reference's frame buffer beside the three arrays
        r = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, want_fb=True)
        assert _said(capfd)[0] == ["generic"]
        _assert_replay(r, ref)
        fb, want = _np(r["fb"]).view(oracle.NEIGH_DTYPE).reshape(n, k), ref["fb"].reshape(n, k)
        for field in ("ind", "dist", "numNeighbors", "intersections"):
            assert np.array_equal(fb[field], want[field]), field
        # a start radius per query
        radii = np.random.default_rng(46).choice(np.float32([0.5, 1.0, 2.0]) * np.float32(r0), n).astype(np.float32)
        ref_q = oracle.trueknn_per_query(xyz, k, radii)
        r = eng.solve(k, 1.0, kernel=_lib.KERNEL_TEAM, start_radii=torch.from_numpy(radii))
        assert _said(capfd)[0] == ["generic"]
        _assert_replay(r, ref_q)
        # phases 1 and 2 after a halo selection that marks the points of one half as boundary queries: the interior rows,
        # then the others into the same arrays
        box = np.float32([0.5, -1, -1, 2, 2, 2])
        boundary = tile_sets.inside(xyz, box)
        assert 0 < boundary.sum() < n
        eng.halo_select(box[None, :], [1], 2)
        out = {"idx": torch.full((n, k), -7, dtype=torch.int32, device=eng.device),
               "dist": torch.full((n, k), -7.0, dtype=torch.float32, device=eng.device),
               "intersections": torch.full((n,), -7, dtype=torch.int64, device=eng.device)}
        r = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, out=out, phase=1)
        assert _said(capfd)[0] == ["generic"]
        inner = np.flatnonzero(~boundary)
        assert (_np(out["idx"])[boundary] == -7).all() and (_np(out["intersections"])[boundary] == -7).all()
        assert_rows_equal(_np(out["idx"])[inner], _np(out["dist"])[inner], ref["idx"][inner], ref["dist"][inner])
        assert np.array_equal(_np(out["intersections"])[inner], ref["intersections"][inner])
        r = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM, out=out, phase=2)
        assert _said(capfd)[0] == ["generic"]
        assert_rows_equal(_np(r["idx"]), _np(r["dist"]), ref["idx"], ref["dist"])
        assert np.array_equal(_np(r["intersections"]), ref["intersections"])
        # a measurement knob, even at its default value
        for knob in ("TKNN_TEAM_MERGE", "TKNN_TEAM_LITE", "TKNN_TEAM_EXT"):
            monkeypatch.setenv(knob, "1")
            r = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM)
            monkeypatch.delenv(knob)
            assert _said(capfd)[0] == ["generic"], knob
            _assert_replay(r, ref)
        # ... and none of them: the plain one
        r = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM)
        assert _said(capfd)[0] == ["plain"]
        _assert_replay(r, ref)
    finally:
        eng.close()
