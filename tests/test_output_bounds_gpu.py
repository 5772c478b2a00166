"""Every call's OUTPUT ARRAYS held to the rule that tests/test_engine_state_gpu.py holds the scratch to: nothing written that is not
the call's to write, and nothing left that the call has to write ("State that carries from one call to the next").  The
wrappers allocate their outputs with torch.empty through the instance's handle; in a test process that memory is fresh zeros or,
very often, the block an identical earlier call just freed -- still holding the right answer -- and it is directly followed by
other live tensors.  So a kernel that skips a row, a pad entry, a count or a CSR tail passes every comparison with a spec, and so
does one that writes a whole register list into a narrower row or indexes one row past the end.

Here every engine gets tests/guarded_outputs.py's handle: each output lies between two 64 KiB guards and everything is filled with
one byte before the call.  For every scenario of tests/state_calls.py (the other file's table and GUARDED_ONLY), every tree it
applies to and the query-count variants, with and without the forced fallback, under each of three fill bytes:

| what is asserted                  | how                                                              | catches                                   |
|-----------------------------------|------------------------------------------------------------------|-------------------------------------------|
| a. no stray write                 | every guard and slack byte of every allocation (the spares and   | a list wider than the row written out, a  |
|                                   | the count pass's offsets too) is still the fill                  | row, record or CSR entry past the end     |
| b. no stale word                  | no 4-byte word of an output (byte of a flag array) still equals  | a skipped row, pad entry, count or tail;  |
|                                   | the fill under ALL of 0x00, 0xFF, 0x5A -- no value does          | needs no reference                        |
| c. same answer                    | bit for bit the other file's fresh(); the family's own check     | an output that is read-modified-written:  |
|                                   | against the CPU spec, once per tree and fallback (not per byte)  | its value depends on the fill             |
| d. documented exceptions are exact| NOT_WRITTEN: the regions a header says are not written are still | "not written" is checked, not skipped     |
|                                   | exactly the fill, and nothing else is                            |                                           |
| e. the tree is only read          | export_tree / export_tree_ex before the first and after the last | a call that writes into the tree          |

0x00 hides a missing zero, 0xFF a missing -1 / NaN pad, 0x5A neither.  The guards reach 64 KiB to either side of an output (256 of
the widest rows here, 64 x 4 B); a write farther off is out of this test's reach.
"""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded_outputs as go  # noqa: E402
import state_calls as sc  # noqa: E402
import test_engine_state_gpu as es  # noqa: E402  (fresh, NOT_REPRODUCIBLE, forced, engine: imported, not copied)

pytestmark = pytest.mark.gpu

BYTES = (0x00, 0xFF, 0x5A)


# ---- d. the regions a header documents as not written ------------------------------------------------------------------------------------
def _rows_of_unfinished(g, result, f, t):
    """Rows of idx, dist and intersections whose query kept level -1."""
    left = f["levels"] == -1
    out = {}
    for name in ("idx", "dist", "intersections"):
        words = result[name].element_size() // 4 * int(np.prod(result[name].shape[1:], dtype=np.int64))
        out[g.name_of(result[name])] = np.repeat(left, words)
    return out


def _without_unfinished_rows(f):
    """The flat result with those rows zeroed: they hold what the outputs held before, which is no part of the answer."""
    f = dict(f)
    for name in ("idx", "dist", "intersections"):
        f[name] = f[name].copy()
        f[name][f["levels"] == -1] = 0
    return f


def _behind_the_dendrogram(g, result, f, t):
    """parent behind n + edges, left / right / size behind edges (the arrays are sized for n - 1 records)."""
    n, edges = t["n"], int(f["edges"][0])
    out = {}
    for i, name in enumerate(("parent", "left", "right", "size")):  # (the order in which TrueKNN._linkage_arrays asks for them)
        r = g.by_name("_linkage_arrays#%d" % i)
        assert r.shape == ((2 * n - 1,) if name == "parent" else (n - 1,)) and (r.nbytes == 0 or g.name_of(result[name]) == r.name)
        out[r.name] = np.arange(r.nbytes // 4) >= (n + edges if name == "parent" else edges)
    return out


def _outside_the_segments(g, result, f, t):
    """Of the message buffer: the wire rows of a segment past its count, and of the header rows the two cells the wrapper does not
    set (the library writes no header: 'everything outside the segments')."""
    (messages,) = [r for r in g.records if r.method == "halo_select_fixed" and len(r.shape) == 2]
    cap = t["n"]
    left = np.ones((messages.shape[0], 4), bool)
    at = 0
    for count in f["counts"].tolist():
        left[at, :2] = False
        left[at + 1:at + 1 + min(count, cap)] = False
        at += cap + 1
    return {messages.name: left.reshape(-1)}


# solve(out=...) allocates the outputs it was handed all the same (dict.setdefault evaluates its default) and drops them: in the
# scenarios that hand in their own, sentinel-filled outputs those allocations are nobody's output -- guarded, never written
CALLER_OWNED = {"halo_phases": "solve", "halo_phases_poisoned_between": "solve"}


class Region:
    def __init__(self, scenarios, header, sentence, words, answer=None):
        """words(g, result, f, t): {record name: a boolean per word, documented as not written}; answer(f): the flat result without
        the region, where the wrapper returns it with the rest (None: it returns none of it)."""
        self.scenarios, self.header, self.sentence, self.words, self.answer = scenarios, header, sentence, words, answer


NOT_WRITTEN = (
    Region(("solve_unfinished", "query_unfinished"), "owlknn.h",
           "unfinished queries keep level -1, their rows are not written and info->unfinished counts them", _rows_of_unfinished, _without_unfinished_rows),
    Region(("hdbscan",), "owlknn_hdbscan.h",
           "The linkage arrays hold n + info.edges, info.edges, ... entries; what lies behind them is not written.", _behind_the_dendrogram),
    Region(("halo_select_fixed",), "owlknn.h",
           "The rows of a segment past min(d_counts[peer], d_caps[peer]) are left untouched, as is everything outside the segments.", _outside_the_segments),
)


def _header_text(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return " ".join(re.sub(r"^\s*/?\*+/?", " ", line) for line in f.read().splitlines()).split()


def test_not_written_holds_only_what_a_header_names():
    """A region may stand in the table only with the sentence of a public header that says it is not written, word for word, and for
    scenarios that exist; tknnEmst's tail is no such region (owlknn_emst.h: 'the unused tail up to n - 1 is u = v = -1, w = +inf')."""
    for region in NOT_WRITTEN:
        words, text = region.sentence.split(), _header_text(region.header)
        assert any(text[i:i + len(words)] == words for i in range(len(text) - len(words) + 1)), "%s does not say: %s" % (region.header, region.sentence)
        assert re.search(r"not written|left untouched", region.sentence)
        for name in region.scenarios:
            assert name in sc.GUARDED_BY_NAME, name
    assert len(NOT_WRITTEN) <= 4 and not any("emst" in name for region in NOT_WRITTEN for name in region.scenarios)


def documented(s, g, result, f, t):
    """{record name: a boolean per word} of what the scenario's call documents as not written."""
    out = {}
    for region in NOT_WRITTEN:
        if s.name in region.scenarios:
            out.update(region.words(g, result, f, t))
    return out


def answer(s, f):
    for region in NOT_WRITTEN:
        if s.name in region.scenarios and region.answer is not None:
            f = region.answer(f)
    return f


# ---- a. to d. --------------------------------------------------------------------------------------------------------------------------
def guarded_run(s, t, fallback, byte):
    """(the flat result, {output record: words still the fill}, {record: words documented as not written}, the records' account) of
    the scenario on a fresh engine whose outputs are guarded and filled with the byte; a. asserted on the way."""
    import torch

    eng = es.engine()
    g = go.Guarded(torch, byte)
    eng._torch = g
    try:
        if not s.bare:
            sc.build(eng, t)
        with es.forced(s.fallback, fallback):
            result = s.run(eng, t)
        torch.cuda.synchronize()
        stray = g.stray()
        assert stray == [], "a write outside an output (record, offsets from its first byte): %r of %r" % (stray, g.records)
        f = sc.flat(result)
        outputs = [r for r in g.records if not r.spare and r.method != CALLER_OWNED.get(s.name)]
        filled = {r.name: g.as_filled(r.name, unit=min(4, r.view.element_size())).cpu().numpy() for r in outputs}
        return f, filled, documented(s, g, result, f, t), [(r.name, r.shape, str(r.dtype), r.spare) for r in g.records]
    finally:
        eng.close()


# The trees of the other file's chain that no scenario names: one point (no internal node, outputs of no rows) and 4 097 (257 leaf
# blocks, the last of one point).  The specs are not run at them -- a., b., d. and the fresh engine's bits are what is held there.
EDGE_TREES = ("n1", "n4097")


def trees_of(s):
    """[(tree, whether the family's check against the spec is run there)]"""
    out = [(tname, True) for tname in s.trees + sc.query_trees(s)]
    if s.name in sc.BY_NAME and not s.bare:
        out += [(tname, False) for tname in EDGE_TREES if tname not in s.trees and s.applies(sc.tree(tname))]
    return out


def hold(s, tname, fallback, spec=True):
    t = sc.tree(tname)
    where = "%s on %s%s" % (s.name, tname, ", fallback forced" if fallback else "")
    want = es.fresh(s, tname, fallback)
    stale, account, regions = None, None, None
    for byte in BYTES:
        f, filled, region, records = guarded_run(s, t, fallback, byte)
        # c. the same answer whatever the outputs held before
        bad = sc.differing(answer(s, f), answer(s, want), skip=es.skipped(s) + s.by_spec)
        assert bad == [], "%s, byte 0x%02X: results that depend on what the outputs held: %s" % (where, byte, bad)
        if byte == BYTES[0]:
            if spec:
                s.check(t, f)
            account, regions = records, region
            stale = filled
        else:
            assert records == account, "%s: the allocations differ from run to run" % where
            assert regions.keys() == region.keys() and all(np.array_equal(regions[k], region[k]) for k in region)
            stale = {name: stale[name] & filled[name] for name in stale}
    # b. and d.: exactly the documented words equal the fill word under all three bytes
    wrong = []
    for name, left in stale.items():
        doc = regions.get(name, np.zeros(len(left), bool))
        if len(doc) != len(left) or not np.array_equal(left, doc):
            never = np.flatnonzero(left & ~doc[:len(left)]) if len(doc) >= len(left) else np.flatnonzero(left)
            touched = np.flatnonzero(~left & doc[:len(left)]) if len(doc) >= len(left) else []
            shape = [r for r in account if r[0] == name][0]
            wrong.append("%s %s: %d words never written (first %s), %d documented as not written but written (first %s)"
                         % (name, shape[1:3], len(never), never[:6].tolist(), len(touched), list(touched[:6])))
    assert wrong == [], "%s: %s" % (where, "; ".join(wrong))
    return sum(len(v) for v in stale.values())


@pytest.mark.parametrize("name", [s.name for s in sc.GUARDED])
def test_outputs_are_written_whole_and_nothing_else_is(name):
    s = sc.GUARDED_BY_NAME[name]
    words = 0
    for tname, spec in trees_of(s):
        assert s.applies(sc.tree(tname)), tname
        for fallback in (False, True) if s.fallback else (False,):
            words += hold(s, tname, fallback, spec)
    assert words > 0, "the scenario allocated no output through the engine's handle"


def test_the_guard_sees_what_it_should_on_the_device():
    """The helper on device tensors, with a real call: a word put back to the fill after the call is reported stale, a byte changed
    behind the row is reported stray -- the two reductions work on the GPU as tests/test_guarded_outputs_expectations.py shows on the CPU."""
    import torch

    t = sc.tree("n17ids")
    eng = es.engine()
    g = go.Guarded(torch, 0x5A)
    eng._torch = g
    try:
        sc.build(eng, t)
        r = eng.knn(None, k=3)
        torch.cuda.synchronize()
        assert g.stray() == [] and g.name_of(r["idx"]) == "knn#0" and [x.spare for x in g.records] == [False, False, False, True]
        assert not g.as_filled("knn#0").any() and g.as_filled("knn#0").is_cuda
        r["idx"].view(-1).view(torch.uint8)[4 * 15:4 * 15 + 4] = 0x5A
        assert torch.nonzero(g.as_filled("knn#0")).reshape(-1).tolist() == [15]
        g.by_name("knn#1").buffer[go.GUARD + 17 * 3 * 4] = 0
        assert g.stray() == [("knn#1", [17 * 3 * 4])]
    finally:
        eng.close()


# ---- e. the tree is only read --------------------------------------------------------------------------------------------------------------
def _tree_bits(eng):
    out = {"export_tree." + k: np.array(v) for k, v in eng.export_tree().items()}
    out.update({"export_tree_ex." + k: np.array(v) for k, v in eng.export_tree_ex().items()})
    return out


@pytest.mark.parametrize("tname", ("n1025", "n17ids", "nan700", "n1025b3") + EDGE_TREES)
def test_the_tree_is_only_read(tname):
    """One engine per tree: every scenario that runs on the tree (or on a query-count variant of it), in the table's order, between
    two exports of the tree and its tables."""
    eng = es.engine()
    try:
        sc.build(eng, sc.tree(tname))
        before = _tree_bits(eng)
        ran = 0
        for s in sc.GUARDED:
            for name, _ in trees_of(s):
                if not s.bare and name.split("q")[0] == tname:
                    for fallback in (False, True) if s.fallback else (False,):
                        with es.forced(s.fallback, fallback):
                            s.run(eng, sc.tree(name))
                        ran += 1
        assert ran >= 5
        after = _tree_bits(eng)
        assert sc.differing(after, before) == [], "a call wrote into the tree"
    finally:
        eng.close()
