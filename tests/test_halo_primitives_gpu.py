"""The device side of the sharded driver in-process, against tests/halo_spec.py: tknnHaloSelect (two passes), tknnHaloSelectFixed
(one pass into segments of a given capacity), the boundary marks both leave for tknnSolveEx's phases, tknnSegmentMin and
tknnDbscanAssign.  Every comparison is exact.  tests/test_halo_expectations.py shows on the CPU that the cases are what this table
says.

| case            | input                                                              | catches                                              |
|-----------------|--------------------------------------------------------------------|------------------------------------------------------|
| sizes           | n = 1, 2, 15..17, 255..257, 4 095..4 097, 19 997; NaN rows         | the last leaf block, the last workgroup, the second  |
|                 |                                                                    | workgroup of the block-mask kernel, the sentinels    |
| scattered       | 40 boxes around points, 5 peers, one without boxes                 | the plain selection, a peer with count 0             |
| peers_apart     | 64 peers, boxes for 0, 1, 31, 32, 33, 62, 63                       | 32-bit shifts, the ends of the mask and of the LDS   |
| peers_all       | 64 peers, one box each around one point                            | a row for 64 peers at once: every bit, every counter |
| everything      | [-FLT_MAX, FLT_MAX]^3 and [-inf, inf]^3 for 3 peers                | all rows but the NaN rows, no sentinel record        |
| overlaps        | nested and shifted boxes of one peer, one region for four peers    | a row listed once per peer, and once for each peer   |
| degenerate      | hi == lo on and off a point, lo > hi, NaN bounds, no boxes, 1 peer | closed bounds, empty boxes, empty calls              |
| planar          | z = 0, boxes with z in [0, 0]                                      | a flat block box against a flat box                  |
| ascending, then | one engine: build, select, build, select                           | the mask and cursor buffer grown lazily and kept     |
| descending      |                                                                    |                                                      |
| fixed           | capacities 0, count - 1, count, count + 1, ample; guards, a fill   | the drop branch, exact counts after drops, rows that |
|                 | pattern                                                            | spill into the next segment, writes past the count   |
| marks           | phase-1 solves after each form                                     | the marks of the count pass and of the one-pass form |
| segment_min     | 72 listed (n, layout, values, preset), twice each; strided inputs  | the ballot rounds, left-over lanes, -1 lanes, 64-bit |
|                 |                                                                    | order, the early drop-out on `out`                   |
| assign          | the sets of dbscan_query_spec and n = 1, 2, 255..257, labels up to | every row against brute force, with and without ids  |
|                 | 2**31 - 1 in reversed order                                        |                                                      |
"""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import halo_spec as hs  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xC3  # every byte of a row nobody wrote


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def engine():
    """One engine for the whole module: rebuilt for every case, its lazily grown buffers kept."""
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def bare():
    """An engine without a tree: tknnSegmentMin needs none."""
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    yield eng
    eng.close()


def _build(eng, c):
    eng.build(np.array(c["P"]), np.array(c["ids"]))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_segment(c, p, seg, what):
    """Wire rows of peer p: distinct members of the spec's list, each with the coordinates of the row that carries the id."""
    got = np.ascontiguousarray(seg[:, 3]).view(np.int32)
    assert len(np.unique(got)) == len(got), (what, "a row twice")
    assert np.isin(got, c["lists"][p]).all(), (what, "a row the spec does not select")
    rows = hs.row_of_id(c["ids"])(got)
    assert np.array_equal(_bits(seg[:, :3]), _bits(c["P"][rows])), (what, "coordinates")
    return got


# ---- the two-pass form ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", hs.FAMILIES)
def test_two_pass_selection(engine, family):
    """TrueKNN.halo_select over the sizes in ascending and then descending order on one engine."""
    for n in hs.SELECT_N + hs.SELECT_N[::-1]:
        c = hs.selection_case(family, n)
        _build(engine, c)
        rows, counts = engine.halo_select(np.array(c["boxes"]), np.array(c["box_peer"]), c["npeers"])
        rows = _np(rows)
        what = c["name"]
        assert counts == c["counts"].tolist(), what
        assert rows.shape == (sum(counts), 4), what
        start = 0
        for p in range(c["npeers"]):
            seg = rows[start:start + counts[p]]
            start += counts[p]
            got = _check_segment(c, p, seg, (what, p))
            assert np.array_equal(np.sort(got), c["lists"][p]), (what, p)


# ---- the one-pass form ----------------------------------------------------------------------------------------------------------

GUARD = 2


def _fixed_call(eng, c, caps):
    """tknnHaloSelectFixed through the C entry point into a buffer of the test's own: GUARD rows, peer 0's segment, GUARD rows,
    peer 1's segment, ..., GUARD rows, every byte FILL beforehand.  (buffer (rows, 4) float32, offsets, counts) on the host."""
    import torch

    from owlraytracing_amd import _lib
    dev = eng.device
    offsets = GUARD + np.concatenate([[0], np.cumsum(caps + GUARD)[:-1]]).astype(np.int64)
    total = int(GUARD + (caps + GUARD).sum())
    buf = torch.full((total * 16,), FILL, dtype=torch.uint8, device=dev).view(torch.float32).view(total, 4)
    boxes = torch.from_numpy(np.array(c["boxes"])).to(dev)
    peer = torch.from_numpy(np.array(c["box_peer"])).to(dev)
    caps_dev = torch.from_numpy(np.array(caps)).to(dev)
    offsets_dev = torch.from_numpy(offsets).to(dev)
    counts = torch.full((c["npeers"],), -7, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(eng._lib.tknnHaloSelectFixed(eng._h, ctypes.c_void_p(boxes.data_ptr()), ctypes.c_void_p(peer.data_ptr()), int(len(peer)),
                                                int(c["npeers"]), ctypes.c_void_p(caps_dev.data_ptr()), ctypes.c_void_p(offsets_dev.data_ptr()),
                                                ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(counts.data_ptr()), eng._stream()))
        torch.cuda.current_stream(dev).synchronize()
    return _np(buf), offsets, _np(counts)


_FIXED = hs.fixed_cases()


@pytest.mark.parametrize("at", range(len(_FIXED)), ids=[c["name"] for c, _ in _FIXED])
def test_one_pass_selection_into_fixed_capacities(engine, at):
    """Exact counts although rows were dropped; the first min(count, cap) rows of a segment are distinct members of the spec's list
    (which ones are dropped is unspecified); every other row of the buffer -- the guards, the tail of a segment, a segment of
    capacity 0 -- still holds the fill pattern."""
    c, caps = _FIXED[at]
    _build(engine, c)
    buf, offsets, counts = _fixed_call(engine, c, caps)
    what = c["name"]
    assert np.array_equal(counts, c["counts"]), (what, caps.tolist())
    written = np.zeros(len(buf), bool)
    for p in range(c["npeers"]):
        kept = int(min(c["counts"][p], caps[p]))
        seg = buf[offsets[p]:offsets[p] + kept]
        _check_segment(c, p, seg, (what, p, int(caps[p])))
        written[offsets[p]:offsets[p] + kept] = True
    rest = buf[~written].view(np.uint8)
    assert (rest == FILL).all(), (what, "rows outside the first min(count, cap) of a segment were written",
                                  np.flatnonzero(~written)[(rest != FILL).any(axis=1)][:8].tolist())
    assert (~written).sum() >= GUARD * (c["npeers"] + 1)


def test_one_pass_selection_through_the_wrapper(engine):
    """TrueKNN.halo_select_fixed: message p starts at the running sum of caps + 1, its header cells carry the exact count, the
    rows follow."""
    from owlraytracing_amd import distributed
    c = hs.selection_case("scattered", 4097)
    caps = hs.capacities(c["counts"], 1)
    assert (caps < c["counts"]).any() and (caps > c["counts"]).any()
    _build(engine, c)
    messages, starts, counts = engine.halo_select_fixed(np.array(c["boxes"]), np.array(c["box_peer"]), c["npeers"], caps.tolist())
    messages = _np(messages)
    assert list(starts) == (np.cumsum(caps + 1) - (caps + 1)).tolist() and len(messages) == int((caps + 1).sum())
    assert np.array_equal(_np(counts), c["counts"])
    for p in range(c["npeers"]):
        head = messages[starts[p]]
        assert distributed._count_of_cells(head[0], head[1]) == c["counts"][p], p
        kept = int(min(c["counts"][p], caps[p]))
        _check_segment(c, p, messages[starts[p] + 1:starts[p] + 1 + kept], ("wrapper", p))


# ---- the boundary marks ---------------------------------------------------------------------------------------------------------

def _count_pass(eng, c):
    import torch

    from owlraytracing_amd import _lib
    dev = eng.device
    boxes = torch.from_numpy(np.array(c["boxes"])).to(dev)
    peer = torch.from_numpy(np.array(c["box_peer"])).to(dev)
    counts = torch.empty((c["npeers"],), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(eng._lib.tknnHaloSelect(eng._h, ctypes.c_void_p(boxes.data_ptr()) if len(peer) else None,
                                           ctypes.c_void_p(peer.data_ptr()) if len(peer) else None, int(len(peer)), int(c["npeers"]),
                                           ctypes.c_void_p(counts.data_ptr()), None, None, eng._stream()))
    return _np(counts)


def _write_pass(eng, c):
    import torch

    from owlraytracing_amd import _lib
    dev = eng.device
    boxes = torch.from_numpy(np.array(c["boxes"])).to(dev)
    peer = torch.from_numpy(np.array(c["box_peer"])).to(dev)
    offsets = torch.from_numpy(np.cumsum(c["counts"]) - c["counts"]).to(dev)
    rows = torch.empty((int(c["counts"].sum()), 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(eng._lib.tknnHaloSelect(eng._h, ctypes.c_void_p(boxes.data_ptr()), ctypes.c_void_p(peer.data_ptr()), int(len(peer)),
                                           int(c["npeers"]), None, ctypes.c_void_p(offsets.data_ptr()), ctypes.c_void_p(rows.data_ptr()),
                                           eng._stream()))
        torch.cuda.current_stream(dev).synchronize()


MARK_K, MARK_R0, MARK_ROUNDS = 3, 0.05, 24  # (0.05 * 2**23 covers the unit cube many times: every row without a NaN finishes)


def _left_at_the_sentinel(eng, n):
    """Which rows a phase-1 solve does NOT write -- tknnSolveEx with phase = 1 works on exactly the rows whose mark is 0 -- and
    how many rows it worked on without finishing them."""
    import torch

    from owlraytracing_amd import _lib

    def fill(nbytes, dtype, shape):
        return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=eng.device).view(dtype).view(shape)
    k = MARK_K
    out = {"idx": fill(n * k * 4, torch.int32, (n, k)), "dist": fill(n * k * 4, torch.float32, (n, k)),
           "intersections": fill(n * 8, torch.int64, (n,)), "levels": fill(n * 4, torch.int32, (n,))}
    r = eng.solve(k, MARK_R0, out=out, phase=1, kernel=_lib.KERNEL_TEAM, max_rounds=MARK_ROUNDS, allow_unfinished=True, want_levels=True)
    idx = _np(out["idx"]).view(np.uint8).reshape(n, -1)
    dist = _np(out["dist"]).view(np.uint8).reshape(n, -1)
    left = (idx == 0xA5).all(axis=1)
    assert np.array_equal(left, (dist == 0xA5).all(axis=1))
    return left, r["info"]["unfinished"]


@pytest.mark.parametrize("family,n", [("scattered", 4097), ("everything_inf", 257)])
def test_boundary_marks_of_both_forms(engine, family, n):
    """The rows a phase-1 solve leaves alone are the spec's boundary rows: after the count pass, unchanged by the write pass that
    follows, after the one-pass form with ample capacities and with every capacity 0 (a dropped row is a boundary row all the
    same).  A row with a NaN is in no box, so it is an interior query -- one that finds nobody: it is worked on and left
    unfinished, which is how its mark of 0 shows.  Before each form the marks are set to another state (no boxes: all 0)."""
    c = hs.selection_case(family, n)
    empty = hs.selection_case("no_boxes", n)
    nan = np.isnan(c["P"]).any(axis=1)
    assert nan.any() and not c["boundary"][nan].any() and np.array_equal(empty["P"].view(np.uint32), c["P"].view(np.uint32))
    assert c["boundary"].any()
    want_left = c["boundary"] | nan
    _build(engine, c)

    def check(what):
        left, unfinished = _left_at_the_sentinel(engine, n)
        assert np.array_equal(left[~nan], c["boundary"][~nan]), (c["name"], what, "rows without a NaN", int((left != want_left).sum()))
        assert np.array_equal(left, want_left) and unfinished == int(nan.sum()), (c["name"], what, "rows with a NaN", unfinished)

    def clear():
        assert (_count_pass(engine, empty) == 0).all()
        left, unfinished = _left_at_the_sentinel(engine, n)
        assert np.array_equal(left, nan) and unfinished == int(nan.sum()), (c["name"], "no boxes: every row is interior")

    clear()
    assert np.array_equal(_count_pass(engine, c), c["counts"])
    check("count pass")
    _write_pass(engine, c)
    check("write pass after the count pass")
    clear()
    _, _, counts = _fixed_call(engine, c, 2 * c["counts"] + 3)
    assert np.array_equal(counts, c["counts"])
    check("one pass, ample capacities")
    clear()
    _, _, counts = _fixed_call(engine, c, 0 * c["counts"])
    assert np.array_equal(counts, c["counts"])
    check("one pass, every capacity 0")


# ---- tknnSegmentMin -------------------------------------------------------------------------------------------------------------

def _segment_min(bare, c, what):
    import torch
    dev = bare.device
    seg, val = torch.from_numpy(c["segment"]).to(dev), torch.from_numpy(c["value"]).to(dev)
    out = torch.from_numpy(c["out"].copy()).to(dev)
    back = bare.segment_min(seg, val, out)
    assert back is out
    got = _np(out)
    assert got.dtype == np.int64 and np.array_equal(got, c["want"]), (what, np.flatnonzero(got != c["want"])[:8].tolist())
    bare.segment_min(seg, val, out)
    assert np.array_equal(_np(out), c["want"]), (what, "a second call changed out")
    assert np.array_equal(_np(seg), c["segment"]) and np.array_equal(_np(val), c["value"]), (what, "inputs written")


@pytest.mark.parametrize("n", hs.SEGMENT_N)
def test_segment_min(bare, n):
    combos = [c for c in hs.segment_combos() if c[0] == n]
    assert len(combos) == len(hs.LAYOUTS)
    for combo in combos:
        c = hs.segment_case(*combo)
        if n == 0:
            assert np.array_equal(c["want"], c["out"])  # (out comes back untouched)
        _segment_min(bare, c, combo)


def test_segment_min_of_strided_inputs(bare):
    """segment and value as every second element of longer tensors; the elements between them would change the result."""
    import torch
    dev = bare.device
    c = hs.segment_case(257, "mixed", "negative", "max")
    seg2 = np.full(2 * 257, 1, np.int32)
    val2 = np.full(2 * 257, hs.I64_MIN, np.int64)
    seg2[::2], val2[::2] = c["segment"], c["value"]
    seg, val = torch.from_numpy(seg2).to(dev)[::2], torch.from_numpy(val2).to(dev)[::2]
    assert not seg.is_contiguous() and not val.is_contiguous()
    out = torch.from_numpy(c["out"].copy()).to(dev)
    bare.segment_min(seg, val, out)
    assert np.array_equal(_np(out), c["want"])


# ---- tknnDbscanAssign -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_ids", [False, True], ids=["rows", "ids"])
@pytest.mark.parametrize("name", hs.ASSIGN_SETS)
def test_dbscan_assign_on_every_row(engine, name, with_ids):
    """Core rows keep their label, every other row takes the smallest label among the core points within eps -- brute force over
    all pairs --, by row whether the tree was built with ids or not."""
    import torch
    c = hs.assign_case(name)
    engine.build(np.array(c["P"]), np.array(c["ids"]) if with_ids else None)
    got = _np(engine.dbscan_assign(c["eps"], torch.from_numpy(np.array(c["core_label"])).to(engine.device)))
    core = c["core"]
    assert got.dtype == np.int32 and np.array_equal(got[core], c["core_label"][core]), (name, "core rows")
    bad = np.flatnonzero(got != c["want"])
    assert len(bad) == 0, (name, len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), c["want"][bad[:8]].tolist())
