"""The tester tested, without a GPU: tests/guarded_outputs.py hands out the views it was asked for, reports a byte written on
either side of one with its offset, and tells a word that was never written from one that was, under each of the three fill bytes.
And the coverage rule, read from the source: every TrueKNN method that allocates an output is the call of a scenario that
tests/test_output_bounds_gpu.py runs, or stands in a short list with its reason -- a wrapper added later cannot escape silently."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded_outputs as go  # noqa: E402
import state_calls as sc  # noqa: E402

BYTES = (0x00, 0xFF, 0x5A)

# TrueKNN methods that call torch.empty and are no scenario's call: the name and why
NOT_A_CALL = {
    "_linkage_arrays": "the allocation shared by linkage, hdbscan_labels and hdbscan: guarded through each of them",
    "_match": "the one library call under match_features, which is a scenario: guarded through it",
}


class Wrapper:
    """What a TrueKNN method does with its handle."""

    def __init__(self, fill):
        self._torch = go.Guarded(torch, fill)

    def some_call(self, shape, dtype):
        torch = self._torch
        return torch.empty(shape, dtype=dtype, device="cpu")

    def other_call(self, count):
        return self._torch.empty(count, dtype=self._torch.int64, device="cpu")

    def call_with_a_spare(self, m):
        torch = self._torch
        out = {"labels": torch.empty((m,), dtype=torch.int32, device="cpu")}
        spare = torch.empty((1,), dtype=torch.int32, device="cpu") if m == 0 else None
        return out, spare


@pytest.mark.parametrize("fill", BYTES)
def test_a_view_is_what_was_asked_for(fill):
    w = Wrapper(fill)
    for shape, dtype in (((7, 5), torch.int32), ((1025, 64), torch.float32), ((3,), torch.int64), ((33,), torch.uint8), ((5, 3, 3), torch.float32),
                         ((9,), torch.float64)):
        v = w.some_call(shape, dtype)
        assert tuple(v.shape) == shape and v.dtype == dtype and v.is_contiguous() and v.data_ptr() % go.ALIGN == 0
        assert (v.view(-1).view(torch.uint8) == fill).all(), "the interior is filled too"
    v = w.other_call(4)  # a bare count, as halo_select asks
    assert tuple(v.shape) == (4,) and v.dtype == torch.int64
    for shape in ((0,), (0, 3), (5, 0)):
        z = w.some_call(shape, torch.float32)
        assert tuple(z.shape) == shape and z.numel() == 0
    g = w._torch
    assert [r.method for r in g.records] == ["some_call"] * 6 + ["other_call"] + ["some_call"] * 3
    assert [r.name for r in g.records][:2] == ["some_call#0", "some_call#1"] and g.records[6].name == "other_call#0"
    assert g.records[0].nbytes == 7 * 5 * 4 and g.records[0].buffer.numel() == 2 * go.GUARD + 256 and g.records[1].buffer.numel() == 2 * go.GUARD + 1025 * 64 * 4
    assert g.name_of(v) == "other_call#0" and g.name_of(g.records[1].view[1000:]) == "some_call#1" and g.name_of(torch.zeros(3)) is None
    assert g.stray() == []
    # the address a wrapper keeps for empty tensors is told from an output by the source line that asked
    w.call_with_a_spare(0)
    assert [(r.method, r.spare, r.shape) for r in g.records[-2:]] == [("call_with_a_spare", False, (0,)), ("call_with_a_spare", True, (1,))]
    assert not any(r.spare for r in g.records[:-1])
    # everything else is torch's own
    assert g.float32 is torch.float32 and g.Tensor is torch.Tensor and isinstance(v, g.Tensor) and g.zeros(2).sum() == 0


@pytest.mark.parametrize("fill", BYTES)
@pytest.mark.parametrize("dtype", (torch.int32, torch.int64, torch.uint8), ids=str)
def test_a_stray_byte_is_reported_with_its_offset(fill, dtype):
    size = torch.empty((), dtype=dtype).element_size()
    other = fill ^ 0x81
    for what in ("element before", "element after", "far end in front", "far end behind", "slack"):
        w = Wrapper(fill)
        w.some_call((4,), torch.float32)  # a bystander that stays clean
        v = w.some_call((5, 7), dtype)
        g = w._torch
        r = g.by_name("some_call#1")
        assert r.nbytes == 35 * size
        v.fill_(1)  # writing the whole interior is no stray write
        assert g.stray() == []
        at = {"element before": -size, "element after": r.nbytes, "far end in front": -go.GUARD, "far end behind": -(-r.nbytes // 256) * 256 + go.GUARD - 1,
              "slack": r.nbytes + 1}[what]
        r.buffer[go.GUARD + at] = other
        assert g.stray() == [("some_call#1", [at])], what
    # several bytes, on both sides, in order; a limit on how many are listed
    r.buffer[go.GUARD - 3] = other
    r.buffer[go.GUARD + r.nbytes + 300] = other
    assert g.stray() == [("some_call#1", [-3, at, r.nbytes + 300])] and g.stray(limit=1) == [("some_call#1", [-3])]


@pytest.mark.parametrize("fill", BYTES)
def test_an_unwritten_word_is_told_from_a_written_one(fill):
    w = Wrapper(fill)
    v = w.some_call((6, 4), torch.int32)
    v[:] = torch.arange(24, dtype=torch.int32).view(6, 4) + 1
    left = torch.zeros(24, dtype=torch.bool)
    assert torch.equal(w._torch.as_filled("some_call#0"), left)
    w = Wrapper(fill)
    v = w.some_call((6, 4), torch.int32)
    rows = torch.tensor([0, 1, 2, 4, 5])
    v[rows] = torch.arange(20, dtype=torch.int32).view(5, 4) + 1  # row 3 is skipped
    v[5, 3] = int(np.uint32(go.fill_word(fill)).astype(np.int32))  # a value that happens to equal this fill's word: told apart by the other fills only
    left[12:16] = True
    left[23] = True
    assert torch.equal(w._torch.as_filled("some_call#0"), left)
    # the 8-byte types by 4-byte words, the byte-sized flags by bytes; an odd size ends in a word that is part slack
    d = w.some_call((3,), torch.float64)
    d[0], d[2] = 1.5, -2.0
    assert w._torch.as_filled("some_call#1").tolist() == [fill == 0, False, True, True, fill == 0, False]
    f = w.some_call((6,), torch.uint8)
    f[:] = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8)
    f5 = w._torch.by_name("some_call#2").buffer
    f5[go.GUARD + 4] = fill  # byte 4 as it was found
    assert w._torch.as_filled("some_call#2", unit=1).tolist() == [False, fill == 0, False, False, True, False]
    assert w._torch.as_filled("some_call#2").shape == (2,)


def test_no_value_survives_all_three_fills():
    """What the GPU test rests on: a word that equals the fill word under all three bytes was not written -- no value does."""
    words = {go.fill_word(b) for b in BYTES}
    assert len(words) == 3
    for value in (0, -1, 1, 0x5A5A5A5A):
        assert sum((value & 0xFFFFFFFF) == wd for wd in words) <= 1


# ---- the coverage rule -----------------------------------------------------------------------------------------------------------------
def allocating_methods():
    """The TrueKNN methods whose body calls `torch.empty`, read from the source."""
    with open(os.path.join(ROOT, "owlraytracing_amd", "trueknn.py")) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "TrueKNN")
    out = []
    for fn in cls.body:
        if isinstance(fn, ast.FunctionDef):
            for node in ast.walk(fn):
                if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "empty"
                        and isinstance(node.func.value, (ast.Name, ast.Attribute)) and (getattr(node.func.value, "id", None) == "torch" or getattr(node.func.value, "attr", None) == "_torch")):
                    out.append(fn.name)
                    break
    return out


def test_every_allocating_method_is_guarded_or_excused():
    methods = allocating_methods()
    assert len(methods) >= 30 and {"solve", "knn", "mean_shift_modes", "ransac", "_match"} <= set(methods), "the reader reads the source"
    calls = {s.call for s in sc.GUARDED}
    missing = [m for m in methods if m not in calls and m not in NOT_A_CALL]
    assert missing == [], "TrueKNN methods that allocate outputs and are no scenario's call (tests/state_calls.py): add a scenario"
    assert len(NOT_A_CALL) <= 3 and all(len(reason) > 20 and "\n" not in reason for reason in NOT_A_CALL.values())
    for name in NOT_A_CALL:
        assert name in methods and name not in calls, "%s: an excuse that is not needed any more" % name


def test_every_wrapper_takes_the_handle_from_the_instance():
    """`torch = self._torch` at the top, never a module-level torch: the guard replaces the instance's handle and nothing else."""
    with open(os.path.join(ROOT, "owlraytracing_amd", "trueknn.py")) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "TrueKNN")
    imported = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom)) and any(a.name.split(".")[0] == "torch" for a in n.names)]
    assert imported == [], "trueknn.py imports torch at module level: TrueKNN's methods could reach it past the instance's handle"
    for fn in cls.body:
        if isinstance(fn, ast.FunctionDef) and fn.name in allocating_methods():
            first = [n for n in ast.walk(fn) if isinstance(n, ast.Assign) and len(n.targets) == 1 and getattr(n.targets[0], "id", None) == "torch"]
            assert first and all(isinstance(a.value, ast.Attribute) and a.value.attr == "_torch" for a in first), fn.name


def test_the_scenarios_only_the_guarded_test_reads():
    names = [s.name for s in sc.GUARDED]
    assert len(set(names)) == len(names) and not set(s.name for s in sc.GUARDED_ONLY) & set(sc.BY_NAME)
    for k in sc.ROW_KS:
        for family in ("solve_lane", "solve_wave", "solve_team", "query", "radius_knn", "knn", "knn_own", "periodic_knn", "batch_knn", "local_pca"):
            s = sc.GUARDED_BY_NAME["%s_k%d" % (family, k)]
            assert s.k == k and all(sc.tree(tname)["n"] == 1025 for tname in s.trees)
    for name in sc.TAKES_QUERIES:
        assert len(sc.query_trees(sc.BY_NAME[name])) == 3
    base = sc.tree("n1025")
    for m in sc.QUERY_COUNTS:
        t = sc.tree("n1025q%d" % m)
        assert t["name"] == "n1025q%d" % m and t["P"] is base["P"] and len(t["Q"]) == m and np.array_equal(t["Q"], base["Q"][:m], equal_nan=True)
        assert np.array_equal(t["qbatch"], base["qbatch"][:m]) and len(t["Qf"]) == (~np.isnan(t["Q"]).any(axis=1)).sum()
    assert sc.tree("n1025b3q65")["batch"] is sc.tree("n1025b3")["batch"]
