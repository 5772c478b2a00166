"""The LBVH builder (owlraytracing_amd/csrc/lbvh.hip) against tests/lbvh_spec.py, every word of every exported array:
sorted keys, order and its inverse, point records with their sentinels, scene box, every node (box, split, other), both
rope arrays, split_owner, and the wide pyramid the team kernels descend -- for point trees (TrueKNN.export_tree_ex, own
and halo tree) and box trees (trueknn.debug_box_tree, with a refit).  Nothing is approximate: a box is a min / max, a key
is a chain of single correctly rounded fp32 operations (-ffp-contract=off on both sides), so every comparison is
lbvh_spec.compare, i.e. np.array_equal on integer views.  tests/test_lbvh_expectations.py holds the specification itself
against brute force without a GPU.

Sizes: 16 / 17 (a full / a short last block of 16), 1024 / 1025 (a second wide level appears above 64 blocks), 4095 / 4097
(a node range that crosses a 4096 boundary of the table pyramid), 65 536 / 65 537 (a third wide level above 4096 blocks),
262 145 (the root's range holds one whole aligned run of 262 144: table level 3 of fit_kernel's range query).
Not covered: fit_kernel's level-4 branch, which needs n > 64^4 = 16.7 M points."""
import numpy as np
import pytest

import lbvh_spec as ls
from owlraytracing_amd import _lib, datasets

pytestmark = pytest.mark.gpu

CURVES = {"hilbert": ls.HILBERT, "morton": ls.MORTON}
POINT_FIELDS = ("n", "curve", "nan_count", "scene", "keys", "prim_id", "row_slot", "points", "nodes", "rope_node", "rope_leaf",
                "split_owner", "wide_levels", "wide_count", "wide_boxes")
BOX_FIELDS = ("prim_id", "nodes", "rope_node", "rope_leaf", "sorted_boxes")
E_STATE = -3


def _engine():
    from owlraytracing_amd.trueknn import TrueKNN
    return TrueKNN()


def _mixture(n, seed=21):
    """A Gaussian mixture with a run of 200 identical points (fewer where n is small): equal keys, split by position."""
    xyz = datasets.gaussian_mixture3d(n, components=8, sigma=0.02, seed=seed)
    run = min(200, n // 3)
    xyz[n // 2: n // 2 + run] = xyz[0]
    return xyz


def _slab(n, seed=22):
    """The same in a plane: one axis of the scene box is degenerate."""
    xyz = _mixture(n, seed)
    xyz[:, 2] = np.float32(0.375)
    return xyz


def _check_points(eng, xyz, curve, ids=None):
    eng.build(xyz, ids)
    got = eng.export_tree_ex()
    want = ls.build_points(xyz, ids=ids, curve=curve)
    wrong = ls.compare(got, want, POINT_FIELDS)
    assert not wrong, "the builder's arrays differ from the specification in %s" % wrong
    return got


@pytest.mark.parametrize("curve", list(CURVES))
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 1023, 1024, 1025, 4095, 4097, 65_536, 65_537, 262_145])
def test_point_tree_equals_the_specification(n, curve, monkeypatch):
    monkeypatch.setenv("TKNN_CURVE", curve)
    eng = _engine()
    try:
        for xyz in (_mixture(n), _slab(n)):
            _check_points(eng, xyz, CURVES[curve])
    finally:
        eng.close()


@pytest.mark.parametrize("curve", list(CURVES))
def test_device_key_equals_host_key(curve, monkeypatch):
    """The sort key is computed once on the device (the tree) and once on the host (tknnQuery's query order, the block-list
    model of tests/test_curve_key.py); both are curve_point_key.  Scenes whose scale cells / ext is not a power of two, a tiny
    and a huge one."""
    monkeypatch.setenv("TKNN_CURVE", curve)
    base = np.random.default_rng(23).random((65_537, 3), dtype=np.float32)
    eng = _engine()
    try:
        for scale, shift in ((3.7, -1.3), (1e-20, 0.0), (3e19, 7e18), (1.0 / 3.0, 1000.0)):
            xyz = (base * np.float32(scale) + np.float32(shift)).astype(np.float32)
            eng.build(xyz)
            got = eng.export_tree_ex()
            want = ls.build_points(xyz, curve=CURVES[curve])
            assert not ls.compare(got, want, ("scene", "keys", "prim_id")), (scale, shift)
    finally:
        eng.close()


# ---- special inputs at n = 1025 ----
N_SPECIAL = 1025


def _with_nans():
    xyz = _mixture(N_SPECIAL, seed=24)
    rows = np.sort(np.random.default_rng(25).choice(N_SPECIAL, 37, replace=False))
    for j, r in enumerate(rows):
        xyz[r, [[0], [1], [2], [0, 1], [1, 2], [0, 2], [0, 1, 2]][j % 7]] = np.nan
    return xyz, rows


@pytest.mark.parametrize("curve", list(CURVES))
def test_nan_points_sort_last_and_widen_nothing(curve, monkeypatch):
    monkeypatch.setenv("TKNN_CURVE", curve)
    xyz, rows = _with_nans()
    eng = _engine()
    try:
        got = _check_points(eng, xyz, CURVES[curve])
    finally:
        eng.close()
    n = N_SPECIAL
    assert got["nan_count"] == 37
    assert np.array_equal(got["prim_id"][n - 37:], rows), "the NaN points are not the last slots in input order"
    assert np.all(got["points"][n - 37: n, :3] == ls.NAN_BITS) and np.array_equal(got["points"][n - 37: n, 3].view(np.int32), rows)
    assert not np.isnan(got["nodes"][:, [0, 1, 2, 4, 5, 6]].view(np.float32)).any() and not np.isnan(got["wide_boxes"]).any()
    clean = np.delete(xyz, rows, axis=0)
    assert np.array_equal(got["scene"], np.concatenate([clean.min(0), clean.max(0)]))
    assert np.array_equal(got["nodes"][0, [0, 1, 2, 4, 5, 6]].view(np.float32), got["scene"])


def _all_nan():
    return np.full((N_SPECIAL, 3), np.nan, np.float32)


def _one_inf():
    xyz = _mixture(N_SPECIAL, seed=26)
    xyz[400, 1] = np.inf
    return xyz


def _identical():
    return np.tile(np.array([[0.25, -3.5, 1e-3]], np.float32), (N_SPECIAL, 1))


@pytest.mark.parametrize("curve", list(CURVES))
@pytest.mark.parametrize("make", [_all_nan, _one_inf, _identical], ids=["all_nan", "one_inf", "identical"])
def test_sets_whose_keys_are_all_equal(make, curve, monkeypatch):
    """No key tells two points apart: the order is the input order and the tree is the tree of the positions."""
    monkeypatch.setenv("TKNN_CURVE", curve)
    xyz = make()
    eng = _engine()
    try:
        got = _check_points(eng, xyz, CURVES[curve])
    finally:
        eng.close()
    assert np.array_equal(got["prim_id"], np.arange(N_SPECIAL)) and len(np.unique(got["keys"])) == 1
    assert got["keys"][0] == (np.uint64(1) << np.uint64(63) if make is _all_nan else 0)
    assert got["nan_count"] == (N_SPECIAL if make is _all_nan else 0)
    assert np.array_equal(got["nodes"][0, [3, 7]].view(np.int32), [1023, 1024])  # the root splits 1025 positions at bit 10


# ---- caller ids, halo tree ----
def test_caller_ids_own_tree_and_halo_tree(monkeypatch):
    monkeypatch.delenv("TKNN_CURVE", raising=False)
    rng = np.random.default_rng(27)
    xyz, halo = _mixture(4097, seed=28), _mixture(1025, seed=29) + np.float32(0.5)
    ids = (rng.permutation(4097) + 2**30).astype(np.int32)
    halo_ids = (rng.permutation(1025) + 2**30 + 4097).astype(np.int32)
    eng = _engine()
    try:
        with pytest.raises(_lib.TknnError) as e:
            eng.export_tree_ex()
        assert e.value.code == E_STATE
        got = _check_points(eng, xyz, ls.HILBERT, ids=ids)
        assert np.array_equal(got["points"][:4097, 3].view(np.int32), ids[got["prim_id"]])
        assert np.array_equal(got["row_slot"][got["prim_id"]], np.arange(4097))
        with pytest.raises(_lib.TknnError) as e:
            eng.export_tree_ex(halo=True)
        assert e.value.code == E_STATE
        eng.set_halo(halo, halo_ids)
        got = eng.export_tree_ex(halo=True)
        wrong = ls.compare(got, ls.build_points(halo, ids=halo_ids), POINT_FIELDS)
        assert not wrong, "the halo tree differs from the specification in %s" % wrong
        assert np.array_equal(got["points"][:1025, 3].view(np.int32), halo_ids[got["prim_id"]])
        assert np.array_equal(got["row_slot"][got["prim_id"]], np.arange(1025))
        assert not ls.compare(eng.export_tree_ex(), ls.build_points(xyz, ids=ids), POINT_FIELDS), "set_halo touched the own tree"
        eng.set_halo()
        with pytest.raises(_lib.TknnError) as e:
            eng.export_tree_ex(halo=True)
        assert e.value.code == E_STATE
    finally:
        eng.close()


# ---- rebuilds on one engine ----
def _rows(eng, xyz, queries):
    n, k = len(xyz), 5
    r0 = datasets.start_radius(n, k)
    solved, asked = eng.solve(k, r0), eng.query(queries, k, r0, want_levels=True)
    out = {"solve_" + name: solved[name].cpu().numpy() for name in ("idx", "dist", "intersections")}
    out.update({"query_" + name: asked[name].cpu().numpy() for name in ("idx", "dist", "intersections", "levels")})
    return out


def test_rebuild_on_the_same_engine_equals_a_fresh_engine(monkeypatch):
    """A smaller build after a larger one keeps the larger one's arrays: stale upper pyramid levels, sentinels and table
    entries must not be read."""
    monkeypatch.delenv("TKNN_CURVE", raising=False)
    queries = np.random.default_rng(30).random((64, 3), dtype=np.float32)
    old = _engine()
    try:
        for n in (65_537, 1025, 17, 4097):
            xyz = _mixture(n, seed=31 + n)
            old.build(xyz)
            got = old.export_tree_ex()
            fresh = _engine()
            try:
                fresh.build(xyz)
                want = fresh.export_tree_ex()
                wrong = ls.compare(got, want, POINT_FIELDS)
                assert not wrong, "n = %d after a larger build: %s differ from a fresh engine's" % (n, wrong)
                rows_want = _rows(fresh, xyz, queries)
            finally:
                fresh.close()
            wrong = ls.compare(got, ls.build_points(xyz), POINT_FIELDS)
            assert not wrong, "n = %d: %s differ from the specification" % (n, wrong)
            wrong = ls.compare(_rows(old, xyz, queries), rows_want)
            assert not wrong, "n = %d after a larger build: rows differ from a fresh engine's in %s" % (n, wrong)
    finally:
        old.close()


# ---- box trees ----
def _boxes(shape, n, seed):
    rng = np.random.default_rng(seed)
    centre = rng.random((n, 3), dtype=np.float32)
    if shape == "mixed":
        half = (np.float32(10.0) ** rng.uniform(-4, -0.7, (n, 3))).astype(np.float32)
    elif shape == "points":
        half = np.zeros((n, 3), np.float32)
    else:  # much larger than their spacing
        half = (np.float32(0.3) + np.float32(0.1) * rng.random((n, 3), dtype=np.float32)).astype(np.float32)
    return np.concatenate([centre - half, centre + half], 1).astype(np.float32)


@pytest.mark.parametrize("curve", list(CURVES))
@pytest.mark.parametrize("shape", ["mixed", "points", "large"])
@pytest.mark.parametrize("n", [1, 2, 64, 65, 4097])
def test_box_tree_and_refit_equal_the_specification(n, shape, curve, monkeypatch):
    from owlraytracing_amd.trueknn import debug_box_tree

    monkeypatch.setenv("TKNN_CURVE", curve)
    boxes = _boxes(shape, n, seed=40 + n)
    if n >= 64:
        boxes[10:30] = boxes[3]  # equal centre keys
    got = debug_box_tree(boxes)
    want = ls.build_boxes(boxes, curve=CURVES[curve])
    wrong = ls.compare(got, want, BOX_FIELDS)
    assert not wrong, "the box tree differs from the specification in %s" % wrong
    assert np.array_equal(got["sorted_boxes"], boxes[got["prim_id"]])
    # moved and resized: same order, same topology, every node box the union of the new boxes
    rng = np.random.default_rng(41 + n)
    moved = _boxes("mixed", n, seed=42 + n) * np.float32(1.5) + rng.normal(0, 1, (1, 6)).astype(np.float32)[:, [0, 1, 2, 0, 1, 2]]
    after = debug_box_tree(boxes, refit=moved)
    wrong = ls.compare(after, ls.build_boxes(boxes, curve=CURVES[curve], refit=moved), BOX_FIELDS)
    assert not wrong, "the refitted box tree differs from the specification in %s" % wrong
    assert not ls.compare(after, got, ("prim_id", "rope_node", "rope_leaf")) and np.array_equal(after["nodes"][:, [3, 7]], got["nodes"][:, [3, 7]])
    assert np.array_equal(after["sorted_boxes"], moved[got["prim_id"]])


def test_refit_without_a_box_tree_is_refused():
    from owlraytracing_amd.trueknn import debug_box_tree

    boxes = _boxes("mixed", 65, seed=43)
    for mode in (1, 2):  # no tree at all; a tree built from points
        with pytest.raises(_lib.TknnError) as e:
            debug_box_tree(boxes, mode=mode)
        assert e.value.code == E_STATE, mode
