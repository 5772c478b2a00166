"""No call may depend on what earlier calls left in the engine.  Every call carves its scratch out of one workspace that only grows
and is never cleared, and shares the device counters, their host copy and a few lists with every other call: a call is right only
if it has written every word of them that it reads ("State that carries from one call to the next").  The scenarios
are tests/state_calls.py's, one per public call; their results are compared BIT FOR BIT with what a fresh engine gives, and
held to the family's own CPU spec as well.

| test                      | the engine before the call                                              | catches                                      |
|---------------------------|-------------------------------------------------------------------------|----------------------------------------------|
| poisoned scratch          | workspace, counters, lists and solve state filled with 0x00, 0xFF, 0x5A | a missing reset (0x00 hides a missing zero,  |
|                           | (tknnDebugPoison), with and without the call's forced fallback          | 0xFF a missing 0xff preset, 0x5A neither)    |
| two fresh engines         | nothing                                                                 | what may be compared bit for bit at all      |
| the chain                 | every other call's leftovers, over five builds, forwards and backwards  | a layout that reads another layout's words   |
| after the largest         | a k = 100 solve; a whole HDBSCAN                                        | ... of the largest and most mixed leftovers  |
| a side stream             | poison on the same stream                                               | a step issued without the caller's stream    |
"""
import contextlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import state_calls as sc  # noqa: E402

pytestmark = pytest.mark.gpu

BYTES = (0x00, 0xFF, 0x5A)
WORKSPACE = 4 << 20  # more than any scenario here needs: the call's layout lies wholly inside the poisoned bytes

# Fields two FRESH engines already give differently, as "call.field": they cannot be compared bit for bit, and are held to the CPU
# spec at the family's tolerance instead (the scenario's check).  What may stand here is limited by name, see the rule below.
NOT_REPRODUCIBLE = (
    # the stability of a condensed cluster is a sum of fp64 terms added with atomicAdd in the order the points' threads arrive
    # (tests/test_hdbscan_gpu.py holds it to 1e-9 relative for that reason)
    "hdbscan.stability",
    "hdbscan_labels.stability",
    # the union pass: a walk that finds its group in the other's set already (an agent-scope atomic read of the lock-free union-find's
    # parents) probes no point pairs, so the pairs tested depend on which unions landed first; the sets, and the labels, do not
    "dbscan.info.point_tests",
    "dbscan.info.union_point_tests",
    "dbscan_auto.info.point_tests",
    "dbscan_auto.info.union_point_tests",
    # a round's walks read the states other walks of the same launch store (relaxed atomics): a dominator decided a moment earlier
    # ends a walk early or decides the point a round sooner -- include/owlknn_nms.h: "info->rounds, point_tests and node_tests are
    # NOT reproducible from call to call"; a round is a hand-over of the undecided points to the next launch
    "radius_nms.info.node_tests",
    "radius_nms.info.point_tests",
    "radius_nms.info.rounds",
)
WORK_COUNTERS = ("node_tests", "point_tests", "skipped_subtrees", "core_point_tests", "union_point_tests", "label_point_tests", "union_node_tests",
                 "lane_rows", "fallback_items", "handed_over")
NEVER = ("idx", "dist", "label", "count", "offset", "parent", "left", "right", "size", "lam", "keep", "cover", "rows", "levels", "core", "noise",
         "intersections", "u", "v", "w", "out", "wsum", "centroid", "cov", "eigen", "normals", "curvature", "edges", "components")


def test_not_reproducible_holds_only_what_may_be_there():
    """Only HDBSCAN's stability, and work counters: never an index, distance, label, count, offset, parent / left / right / size, lambda,
    keep / cover field or a round count of linkage or emst -- one of those that two fresh engines give differently is a finding to
    fix.  The one round count allowed is radius_nms's, the number of hand-overs its header documents as free."""
    calls = {s.call for s in sc.TABLE}
    assert not set(WORK_COUNTERS) & set(NEVER) and "rounds" not in WORK_COUNTERS and "stability" not in WORK_COUNTERS
    for entry in NOT_REPRODUCIBLE:
        call, field = entry.split(".", 1)
        last = field.split(".")[-1]
        assert call in calls, entry
        if last == "stability":
            assert call in ("hdbscan", "hdbscan_labels") and field == "stability", entry
        elif last == "rounds":
            assert call == "radius_nms" and field == "info.rounds", entry
        else:
            assert field == "info." + last and last in WORK_COUNTERS, "%s: only HDBSCAN's stability and work counters may be listed" % entry


def skipped(s):
    return tuple(e.split(".", 1)[1] for e in NOT_REPRODUCIBLE if e.split(".", 1)[0] == s.call)


@contextlib.contextmanager
def forced(variable, on):
    """The call's forced-fallback variable set to 1 (it is read at call time), or unset."""
    before = None if variable is None else os.environ.pop(variable, None)
    if variable is not None and on:
        os.environ[variable] = "1"
    try:
        yield
    finally:
        if variable is not None:
            os.environ.pop(variable, None)
            if before is not None:
                os.environ[variable] = before


def engine():
    from owlraytracing_amd.trueknn import TrueKNN

    return TrueKNN(device=0)


def poison(eng, what, byte, stream=None):
    from owlraytracing_amd import _debug_lib

    return _debug_lib.poison(eng, what, byte, WORKSPACE, stream=stream)


def on_a_new_engine(s, t, fallback):
    eng = engine()
    try:
        if not s.bare:
            sc.build(eng, t)
        with forced(s.fallback, fallback):
            return sc.flat(s.run(eng, t))
    finally:
        eng.close()


_FRESH = {}


def fresh(s, tname, fallback=False):
    """What a fresh engine gives for the scenario on the tree: computed once per module, shared, never written."""
    key = (s.name, tname, fallback)
    if key not in _FRESH:
        got = on_a_new_engine(s, sc.tree(tname), fallback)
        for a in got.values():
            a.setflags(write=False)
        _FRESH[key] = got
    return _FRESH[key]


def same_as_fresh(s, tname, got, fallback=False):
    want = fresh(s, tname, fallback)
    bad = sc.differing(got, want, skip=skipped(s))
    for f in bad[:3]:
        if f in got and f in want and got[f].shape == want[f].shape:
            at = np.flatnonzero(sc.bits(got[f]).reshape(-1) != sc.bits(want[f]).reshape(-1))
            print("%s on %s: %s differs in %d bytes/words, first at %d: %r, fresh %r" % (s.name, tname, f, len(at), at[0], got[f].reshape(-1)[:4], want[f].reshape(-1)[:4]))
    return bad


PAIRS = [(s.name, tname) for s in sc.TABLE for tname in s.trees]


def test_the_table_reaches_every_tree_it_names():
    for name, tname in PAIRS:
        assert sc.BY_NAME[name].applies(sc.tree(tname)), (name, tname)
    assert {tname for _, tname in PAIRS} >= {"n1025", "n17ids", "nan700", "n1025b3"}


# ---- (b) what can be compared at all --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tname", PAIRS)
def test_two_fresh_engines_agree(name, tname):
    s, t = sc.BY_NAME[name], sc.tree(tname)
    for fallback in (False, True) if s.fallback else (False,):
        first = fresh(s, tname, fallback)
        second = on_a_new_engine(s, t, fallback)
        assert sc.differing(second, first, skip=skipped(s)) == [], "two fresh engines differ: a finding, or a field for NOT_REPRODUCIBLE"
        s.check(t, first)


# ---- (a) poisoned scratch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", BYTES, ids=["0x00", "0xFF", "0x5A"])
@pytest.mark.parametrize("name,tname", PAIRS)
def test_poisoned_scratch(name, tname, byte):
    from owlraytracing_amd import _debug_lib

    s, t = sc.BY_NAME[name], sc.tree(tname)
    eng = engine()
    try:
        if not s.bare:
            sc.build(eng, t)
        for fallback in (False, True) if s.fallback else (False,):
            assert poison(eng, _debug_lib.POISON_ALL, byte) >= WORKSPACE
            with forced(s.fallback, fallback):
                got = sc.flat(s.run(eng, t))
            assert same_as_fresh(s, tname, got, fallback) == [], "the call read what it had not written (byte 0x%02X%s)" % (byte, ", fallback forced" if fallback else "")
            s.check(t, got)
    finally:
        eng.close()


def test_poison_refusals_and_what_it_fills():
    import ctypes

    from owlraytracing_amd import _debug_lib

    lib = _debug_lib.load()
    E_ARG = -1
    eng = engine()
    try:
        filled = ctypes.c_int64(-7)
        for bad in (dict(e=None), dict(what=16), dict(what=0x80000001), dict(byte=-1), dict(byte=256)):
            a = dict(dict(e=eng._h, what=_debug_lib.POISON_ALL, byte=0x5A), **bad)
            assert lib.tknnDebugPoison(a["e"], a["what"], a["byte"], 0, ctypes.byref(filled), None) == E_ARG, bad
            assert lib.tknnLastError().decode().startswith("tknnDebugPoison"), bad
            assert filled.value == -7, "a refused call writes nothing"
        # a bare engine: the counters, their host copy and the tie list are there; the workspace is grown on request
        small = _debug_lib.poison(eng, _debug_lib.POISON_COUNTERS | _debug_lib.POISON_LISTS, 0xFF)
        assert 0 < small < WORKSPACE
        assert _debug_lib.poison(eng, _debug_lib.POISON_WORKSPACE, 0, min_workspace_bytes=WORKSPACE) == WORKSPACE
        assert _debug_lib.poison(eng, _debug_lib.POISON_SOLVE, 0) == 0, "no tree yet: no per-slot state"
        assert _debug_lib.poison(eng, 0, 0) == 0
        t = sc.tree("n17ids")
        sc.build(eng, t)
        assert _debug_lib.poison(eng, _debug_lib.POISON_SOLVE, 0x5A) == 17 * (1 + 8 + 4) + 20
        # the tree, the ids and the scene are not scratch
        s = sc.BY_NAME["knn"]
        before = sc.flat(s.run(eng, t))
        poison(eng, _debug_lib.POISON_ALL, 0xFF)
        assert sc.differing(sc.flat(s.run(eng, t)), before) == []
    finally:
        eng.close()


# ---- (c) natural garbage ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_engine():
    eng = engine()
    yield eng
    eng.close()


@pytest.mark.parametrize("order", ("table", "reverse"))
def test_chain_over_five_builds(chain_engine, order):
    """The whole table on ONE engine (the second order finds what the first left), each call after whatever the calls before it left
    behind, across builds of 4 097, 17, 1 025 (batched), 1 and 1 025 points: every result is the fresh engine's."""
    eng = chain_engine
    table = sc.TABLE if order == "table" else sc.TABLE[::-1]
    bad, ran = [], 0
    for tname in sc.CHAIN:
        t = sc.tree(tname)
        sc.build(eng, t)
        for s in table:
            if s.applies(t):
                got = sc.flat(s.run(eng, t))
                ran += 1
                bad += [(tname, s.name, f) for f in same_as_fresh(s, tname, got)]
    assert bad == [], "results that depend on the calls before them"
    assert ran > 3 * len(sc.TABLE)


@pytest.mark.parametrize("leader", ("solve_bigk", "hdbscan"))
def test_directly_after_the_largest_leftovers(leader):
    """Each call straight after the call that leaves the largest (a k = 100 solve: 1 025 lists in memory) and the most mixed
    (HDBSCAN: kNN, Boruvka, contraction, condensed tree) leftovers, no build in between."""
    t = sc.tree("n1025")
    eng = engine()
    try:
        sc.build(eng, t)
        bad = []
        for s in sc.TABLE:
            if s.applies(t):
                sc.BY_NAME[leader].run(eng, t)
                bad += [(s.name, f) for f in same_as_fresh(s, "n1025", sc.flat(s.run(eng, t)))]
        assert bad == []
    finally:
        eng.close()


# ---- (d) a real side stream -------------------------------------------------------------------------------------------------------------
def test_on_a_side_stream():
    """Every scenario once on a stream of its own, its inputs made on that stream, poison on the same stream directly before it: a
    step issued on another stream than the caller's (a sort, a scan, a copy) is ordered only by accident on the null stream."""
    import torch

    from owlraytracing_amd import _debug_lib

    for s in sc.TABLE:  # the null-stream results first: nothing else runs beside the side stream
        fresh(s, s.trees[0])
    stream = torch.cuda.Stream(device=0)
    bad = []
    with torch.cuda.stream(stream):
        eng = engine()
        try:
            for tname in sc.TREE_NAMES:
                todo = [s for s in sc.TABLE if s.trees[0] == tname]
                if not todo:
                    continue
                t = sc.tree(tname)
                sc.build(eng, t)
                for s in todo:
                    poison(eng, _debug_lib.POISON_WORKSPACE | _debug_lib.POISON_COUNTERS, 0x5A)
                    bad += [(s.name, f) for f in same_as_fresh(s, tname, sc.flat(s.run(eng, t)))]
            stream.synchronize()
        finally:
            eng.close()
    assert bad == [], "results that differ on a side stream"
