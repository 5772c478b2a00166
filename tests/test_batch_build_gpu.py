"""The batched build (tknnBuildBatched, TrueKNN.build(points, batch=...)) on a GPU: every exported word of the tree against
tests/batch_spec.py's build_points -- tests/lbvh_spec.py's radix tree, node table and wide pyramid rebuilt from the batched
keys --, the batches' slot ranges against numpy lower bounds, a one-batch tree against the plain build, and the existing calls
on a batched tree against what they give on a plain one."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_spec as bs  # noqa: E402
import lbvh_spec as ls  # noqa: E402

pytestmark = pytest.mark.gpu

POINT_FIELDS = ("n", "curve", "nan_count", "scene", "keys", "prim_id", "row_slot", "points", "nodes", "rope_node", "rope_leaf",
                "split_owner", "wide_levels", "wide_count", "wide_boxes")
CURVES = {"hilbert": ls.HILBERT, "morton": ls.MORTON}


def _engine():
    from owlraytracing_amd.trueknn import TrueKNN

    return TrueKNN(device=0)


@pytest.mark.parametrize("curve", list(CURVES))
@pytest.mark.parametrize("num_batches", [7, 33])
def test_batched_tree_equals_the_specification(num_batches, curve, monkeypatch):
    monkeypatch.setenv("TKNN_CURVE", curve)
    P, batch = bs.build_case(num_batches)
    assert (np.diff(batch) < 0).any() and not (batch == 2).any(), "unsorted labels, one empty batch"
    ids = (np.arange(len(P), dtype=np.int32) * 3 + 11)[::-1].copy()
    eng = _engine()
    try:
        for given in (None, ids):
            info = eng.build(P, ids=given, batch=batch, num_batches=num_batches)
            assert info["n"] == len(P)
            got = eng.export_tree_ex()
            want = bs.build_points(P, batch, num_batches, ids=given, curve=CURVES[curve])
            wrong = ls.compare(got, want, POINT_FIELDS)
            assert not wrong, "the batched tree differs from the specification in %s" % wrong
            layout = eng.batch_layout()
            bb = bs.key_bits(num_batches)
            assert layout["num_batches"] == num_batches and layout["key_bits"] == bb
            starts = layout["starts"].cpu().numpy()
            assert starts.dtype == np.int32 and np.array_equal(starts, want["starts"])
            lower = np.searchsorted(got["keys"], np.arange(num_batches + 1, dtype=np.uint64) << np.uint64(63 - bb), side="left")
            assert np.array_equal(starts, lower) and starts[-1] == len(P) - got["nan_count"] and starts[2] == starts[3]
            clean = slice(0, int(starts[-1]))
            assert np.array_equal(got["keys"][clean] >> np.uint64(63 - bb), batch[got["prim_id"][clean]].astype(np.uint64))
        # the default number of batches: the largest label + 1
        eng.build(P, batch=batch)
        assert eng.batch_layout()["num_batches"] == int(batch.max()) + 1
    finally:
        eng.close()


@pytest.mark.parametrize("n", [1, 17, 3000])
def test_one_batch_gives_the_plain_tree_word_for_word(n):
    P = bs.build_case(7)[0][:n]
    eng, plain = _engine(), _engine()
    try:
        eng.build(P, batch=np.zeros(n, np.int32), num_batches=1)
        plain.build(P)
        assert not ls.compare(eng.export_tree_ex(), plain.export_tree_ex(), POINT_FIELDS)
        assert not ls.compare(eng.export_tree(), plain.export_tree())
        layout = eng.batch_layout()
        assert layout["key_bits"] == 0 and layout["starts"].cpu().numpy().tolist() == [0, n - int(np.isnan(P).any(axis=1).sum())]
    finally:
        eng.close(), plain.close()


def test_existing_calls_treat_a_batched_tree_as_one_set():
    """solve on the golden points under random labels gives the golden rows; knn, radius_knn and dbscan give what they give
    on the plain tree."""
    from conftest import assert_rows_match

    g = load_golden("uniform3d_n2048_k5")
    xyz, k, r0 = g["xyz"], int(g["k"]), float(g["start_radius"])
    rng = np.random.default_rng(360)
    batch = rng.integers(0, 5, len(xyz)).astype(np.int32)
    Q = rng.random((200, 3), dtype=np.float32)
    eng, plain = _engine(), _engine()
    try:
        eng.build(xyz, batch=batch, num_batches=5)
        plain.build(xyz)
        assert (eng.export_tree_ex()["prim_id"] != plain.export_tree_ex()["prim_id"]).any(), "another order"
        r = eng.solve(k, r0)
        assert r["info"]["rounds"] == int(g["rounds"])
        assert_rows_match(r["idx"].cpu().numpy(), r["dist"].cpu().numpy(), r["intersections"].cpu().numpy(), g)
        for a, b in ((eng.knn(Q, 10), plain.knn(Q, 10)), (eng.knn(k=10), plain.knn(k=10)), (eng.radius_knn(Q, 7, radius=0.1), plain.radius_knn(Q, 7, radius=0.1))):
            for name in ("idx", "dist", "counts"):
                assert np.array_equal(a[name].cpu().numpy().view(np.int32), b[name].cpu().numpy().view(np.int32)), name
        a, b = eng.dbscan(0.05, 4, want_counts=True), plain.dbscan(0.05, 4, want_counts=True)
        assert np.array_equal(a["core"].cpu().numpy(), b["core"].cpu().numpy()) and np.array_equal(a["counts"].cpu().numpy(), b["counts"].cpu().numpy())
        assert a["info"]["clusters"] == b["info"]["clusters"]
    finally:
        eng.close(), plain.close()
