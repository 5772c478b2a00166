"""The 16-lane team helpers of the TrueKNN kernels on the device, one at a time (tknnDebugTeamLanes, include/owlknn_debug.h),
against tests/team_lanes_spec.py.  Every comparison is bit for bit, but for t_team_sum(float), which owes lane 0's value within
4 * 2^-24 * sum |x| of the float64 sum.  tests/test_team_lanes_expectations.py shows on the CPU that the specification agrees with
brute force and that the cases are what this table says.  A mismatch names the op, the class, the team's position in its wave and
the first differing lane.

| class          | input                                                                   | catches                                          |
|----------------|-------------------------------------------------------------------------|--------------------------------------------------|
| random         | keys over all 64 (32, 96) bits; squares over every binade, denormals, 0,| a wrong exchange of a network, a wrong DPP control|
|                | FLT_MAX, +inf                                                           | word, the root of an edge value                  |
| duplicates     | 1, 2, 3 or 5 distinct distance words per team, random ids, equal keys   | an order the index must decide                   |
| truncated      | SORT16_U32 on (square without its last four bits | lane)                | the words t_sorted_row sorts                     |
| boundary       | squares 17 ulps apart over a truncated word (fast path), 1 ulp across a | the `unsure` rule of t_sorted_row: a pair the    |
|                | word boundary, inside one word, equal, with equal rounded roots; runs   | fast path must not take, one it takes wrongly;   |
|                | of 3 and 4; T from zero over the denormals to the top binade; the larger| FLT_MAX and infinite squares                     |
|                | id on the smaller square; alone, beside 3 and 11 far squares            |                                                  |
| have_masks     | empty, full, each lane, each prefix, 200 masks with holes; NaN squares  | a lane without a candidate that gets into the    |
|                | and any id on the other lanes                                           | row, a prefix assumed                            |
| merge          | NREG 1..4, full 0 / 1, fill 0, 1, 15, 16, 17, 31, 32, lists of 0, 1, 15,| the skip branch at every register, left_out of a |
|                | 16, 17, 16 NREG - 1, 16 NREG entries, candidates below, above, among,   | row that stays out and of one that pushes out,   |
|                | tied with the last entry, from three squares; left_out unset and 0      | the second row, a list with empties              |
| neighbours     | every boundary, have_masks and merge case in each of the four positions | a wave-wide ballot (unsure, take, fill > 16 row) |
|                | of a wave beside three fast-path / three exact-network teams (merge:    | that lets one team's lanes decide for another's  |
|                | three taking teams with fill 32 / three with fill 0), and as 4 copies   |                                                  |
| team_counts    | the first 1, 2, 3, 4, 5, 133 teams of each op's random class            | the lanes of missing teams: their stores, their  |
|                |                                                                         | part in ballots and wave-wide sums               |
| kth, row_ties, | every k; lists of few distances around the radii, empties, left_out at  | the register select, the lane read; tie and edge |
| straddle,      | / above the last word, look off; distances at r, r / sqrt 3, r sqrt 2   | at k, at register borders, with left_out; the    |
| first_level    | give or take ulps; points at a radius of the sequence on one axis       | float32 order of operations                      |
| reduce, moves  | words with +-inf, denormals, a quiet NaN; floats; small integers; masks | a rotation that misses lanes, NaN handling, the  |
|                | all clear, all set, the carry of acc = 0xffffffff, four broadcast lanes | inline v_addc, masked DPP moves, mbcnt           |
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import team_lanes_spec as ts  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(op, variant, inp):
    import torch

    from owlraytracing_amd import _debug_lib

    dev = torch.from_numpy(np.ascontiguousarray(inp, np.uint32).view(np.int32)).to("cuda:0")
    out = _debug_lib.team_lanes(op, variant, dev, inp.shape[0])
    return np.ascontiguousarray(out.cpu().numpy()).view(np.uint32)


def _same(op, variant, cls, got, want, skip_words=(), names=None):
    """bit for bit; else the op, the class, the team with its position in its wave and the first differing word and lane"""
    got, want = got.copy(), want.copy()
    for w in skip_words:
        got[:, w] = want[:, w]
    if np.array_equal(got, want):
        return
    t, w, lane = (int(x[0]) for x in np.nonzero(got != want))
    raise AssertionError("%s variant %d, class %s: team %d%s (position %d of its wave), out word %d, lane %d: got %#x, want %#x; %d teams differ"
                         % (ts.OP_NAMES[op], variant, cls, t, " [%s]" % names[t] if names else "", t & 3, w, lane, got[t, w, lane], want[t, w, lane],
                            int((got != want).any(axis=(1, 2)).sum())))


def _check(op, variant, cls, inp, names=None):
    want = ts.expected(op, variant, inp)
    got = _run(op, variant, inp)
    if op == ts.MERGE:
        got = ts.clamp_left_out(got, variant)
    _same(op, variant, cls, got, want, skip_words=(ts.R_SUM_F32,) if op == ts.REDUCE else (), names=names)
    return got, want


def _check_team_counts(op, variant):
    """class team_counts: the last wave lacks teams; their lanes run the helper and store nothing (the words behind stay 0)"""
    inp = ts.random_cases(op, variant)
    for count in ts.TEAM_COUNTS:
        _check(op, variant, "team_counts=%d" % count, inp[:count])


def _check_neighbours(op, variant, cls, cases, names=None):
    """class neighbours: each case in every position of a wave beside three other teams gives what it gives beside three copies of
    itself, word for word (and both are the specification's)"""
    want = ts.expected(op, variant, cases)
    alone = _run(op, variant, ts.four_copies(cases))
    if op == ts.MERGE:
        alone, want = ts.clamp_left_out(alone, variant), ts.clamp_left_out(want, variant)
    _same(op, variant, cls + ", four copies", alone, np.repeat(want, 4, axis=0), names=None if names is None else [n for n in names for _ in range(4)])
    for beside_name, others in ts.neighbour_sets(op, variant).items():
        teams, at = ts.beside(cases, others)
        got = _run(op, variant, teams)
        if op == ts.MERGE:
            got = ts.clamp_left_out(got, variant)
        for p in range(4):
            _same(op, variant, "%s beside %s, position %d" % (cls, beside_name, p), got[at[:, p]], alone[p::4], names=names)
            _same(op, variant, "%s beside %s, position %d (against the specification)" % (cls, beside_name, p), got[at[:, p]], want, names=names)


@pytest.mark.parametrize("op", [ts.SORT16, ts.CLEAN16, ts.SORT16_U32, ts.SORT16_3, ts.CLEAN16_3], ids=lambda op: ts.OP_NAMES[op])
def test_sorting_networks(op):
    for cls, inp in ts.sort_cases(op).items():
        _check(op, 0, cls, inp)
    _check_team_counts(op, 0)


def test_sorted_row():
    _check(ts.SORTED_ROW, 0, "random", ts.row_random())
    _check(ts.SORTED_ROW, 0, "duplicates", ts.row_duplicates())
    boundary, paths, names = ts.row_boundary()
    _check(ts.SORTED_ROW, 0, "boundary", boundary, names)
    # a fast-path case only takes the fast path if its whole wave does: four copies, and the fast cases among themselves
    fast = boundary[[p == "fast" for p in paths]]
    _check(ts.SORTED_ROW, 0, "boundary, the fast-path cases", fast[:len(fast) // 4 * 4], [n for n, p in zip(names, paths) if p == "fast"])
    _check(ts.SORTED_ROW, 0, "have_masks", ts.row_have_masks())
    _check_neighbours(ts.SORTED_ROW, 0, "boundary", boundary, names)
    _check_neighbours(ts.SORTED_ROW, 0, "have_masks", ts.row_have_masks())
    _check_team_counts(ts.SORTED_ROW, 0)


@pytest.mark.parametrize("nreg", [1, 2, 3, 4])
def test_merge_rows(nreg):
    inp, names = ts.merge_cases(nreg)
    _check(ts.MERGE, nreg, "merge", inp, names)
    _check_neighbours(ts.MERGE, nreg, "merge", inp, names)
    _check_team_counts(ts.MERGE, nreg)


@pytest.mark.parametrize("nreg", [1, 2, 3, 4])
def test_kth_dist(nreg):
    got, _ = _check(ts.KTH, nreg, "random", ts.kth_cases(nreg))
    assert (got == got[:, :, :1]).all(), "every lane of a team has the same word"
    _check_team_counts(ts.KTH, nreg)


@pytest.mark.parametrize("nreg", [1, 2, 3, 4])
def test_row_ties(nreg):
    _check(ts.ROW_TIES, nreg, "row_ties", ts.row_ties_cases(nreg))
    _check_team_counts(ts.ROW_TIES, nreg)


def test_tie_may_straddle():
    _check(ts.STRADDLE, 0, "straddle", ts.straddle_cases())
    _check_team_counts(ts.STRADDLE, 0)


def test_first_level():
    _check(ts.FIRST_LEVEL, 0, "first_level", ts.first_level_cases())
    _check_team_counts(ts.FIRST_LEVEL, 0)


def test_reductions():
    for cls, inp in ts.reduce_cases().items():
        got, want = _check(ts.REDUCE, 0, cls, inp)
        fsum = ts.f32(got[:, ts.R_SUM_F32])
        if cls != "words":  # lane 0 reads the float sum; the order of the additions differs by lane
            total, bound = ts.fsum_bound(inp)
            err = np.abs(fsum[:, 0].astype(np.float64) - total)
            print("t_team_sum(float), class %s: largest error / bound = %.3f" % (cls, float((err / np.maximum(bound, 1e-300)).max())))
            assert (err <= bound).all(), ("REDUCE", cls, "team %d" % int(np.argmax(err > bound)))
        if cls == "small_integers":  # every order of addition is exact
            _same(ts.REDUCE, 0, cls + ", the float sum in all 16 lanes", got[:, ts.R_SUM_F32:ts.R_SUM_F32 + 1], want[:, ts.R_SUM_F32:ts.R_SUM_F32 + 1])
    _check_team_counts(ts.REDUCE, 0)


def test_lane_moves():
    inp = ts.moves_cases()
    for lane in ts.MOVES_BCAST_LANES:
        _check(ts.MOVES, lane, "moves", inp)
        for count in ts.TEAM_COUNTS:  # a broadcast lane in a missing team reads its zero word
            _check(ts.MOVES, lane, "team_counts=%d" % count, inp[:count])


def test_refusals_write_nothing_and_zero_teams_launch_nothing():
    import ctypes

    import torch

    from owlraytracing_amd import _debug_lib

    lib = _debug_lib.load()
    inp = torch.zeros((4, 3, 16), dtype=torch.int32, device="cuda:0")
    out = torch.full((4, 3, 16), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    i, o = ctypes.c_void_p(inp.data_ptr()), ctypes.c_void_p(out.data_ptr())
    for args in ((ts.SORT16_3, 0, None, o, 4), (ts.SORT16_3, 0, i, None, 4), (ts.SORT16_3, 0, i, o, -1), (ts.SORT16_3, 0, i, o, ts.MAX_TEAMS + 1),
                 (13, 0, i, o, 4), (-1, 0, i, o, 4), (ts.SORT16_3, 1, i, o, 4), (ts.MERGE, 0, i, o, 4), (ts.MERGE, 5, i, o, 4), (ts.MOVES, 64, i, o, 4)):
        assert lib.tknnDebugTeamLanes(*args, None) == -1, args
        assert lib.tknnLastError().decode().startswith("tknnDebugTeamLanes: "), args
    assert lib.tknnDebugTeamLanes(ts.SORT16_3, 0, i, o, 0, None) == 0
    torch.cuda.synchronize()
    assert (out == 0x5A5A5A5A).all()
    assert lib.tknnDebugTeamLanes(ts.SORT16_3, 0, i, o, 3, None) == 0  # returns with the stream synchronised
    assert (out[:3] == 0).all() and (out[3] == 0x5A5A5A5A).all(), "the missing team of the wave stores nothing"
