"""TrueKNN.fps (tknnFps, include/owlknn_fps.h) against tests/fps_spec.py: the names, the counts and the bits of the distances are
the brute-force loop's, and point_tests is exactly what the pruning rule, restated over the exported tree, says."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import fps_spec as fs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from owlraytracing_amd.trueknn import TrueKNN

    e = TrueKNN(device=0)
    yield e
    e.close()


def run(eng, S, **kw):
    r = eng.fps(num_samples=S, **kw)
    out = {k: v.cpu().numpy() for k, v in r.items() if k != "info"}
    out["info"] = r["info"]
    return out


def same(got, want, clouds=None):
    rows = slice(None) if clouds is None else list(clouds)
    assert np.array_equal(got["counts"][rows], want["counts"][rows]), "counts differ"
    assert np.array_equal(got["idx"][rows], want["idx"][rows]), "names differ"
    assert np.array_equal(got["dist"][rows].view(np.int32), want["dist"][rows].view(np.int32)), "distances differ in their bits"


def layout(eng):
    return eng.batch_layout()["starts"].cpu().numpy()


def check_both(eng, want, S, starts=None, **kw):
    """The pruned and the unpruned call against ``want``; point_tests of both against the rule over the exported tree."""
    tree = eng.export_tree_ex()
    got = run(eng, S, **kw)
    same(got, want)
    rule = fs.visited_blocks(tree, S, starts=starts, **kw)
    assert np.array_equal(rule["idx"], want["idx"]), "the restated rule itself misses brute force"
    assert got["info"]["point_tests"] == 16 * int(rule["visits"].sum())
    assert got["info"]["samples"] == int(want["counts"].sum()) and got["info"]["bad_starts"] == want["bad_starts"]
    full = run(eng, S, prune=False, **kw)
    same(full, want)
    assert full["info"]["point_tests"] == 16 * int((rule["touching"] * want["counts"]).sum())
    assert got["info"]["point_tests"] <= full["info"]["point_tests"]
    return got


@pytest.mark.parametrize("n,S", [(1, 1), (1, 3), (6, 6), (6, 10), (17, 17), (17, 5)])
def test_trees_without_a_pyramid(eng, n, S):
    P = fs.uniform_case(n, 710)
    eng.build(P)
    want = fs.brute(P, S)
    got = check_both(eng, want, S)
    assert got["counts"][0] == min(n, S) and (got["idx"][0, min(n, S):] == -1).all() and np.isinf(got["dist"][0, min(n, S):]).all()
    assert np.isinf(got["dist"][0, 0]) and got["idx"][0, 0] == 0


def test_three_clouds_one_empty(eng):
    P, batch = fs.tiny_clouds_case()
    eng.build(P, batch=batch, num_batches=3)
    want = fs.brute(P, 8, batch=batch, num_batches=3)
    got = check_both(eng, want, 8, starts=layout(eng))
    assert got["counts"].tolist() == [6, 0, 4] and (got["idx"][1] == -1).all() and np.isinf(got["dist"][1]).all()


def test_clouds_that_straddle_blocks(eng):
    P, batch = fs.straddle_case()
    B = len(fs.STRADDLE_SIZES)
    eng.build(P, batch=batch)
    assert eng.export_tree_ex()["wide_count"][:2].tolist() == [188, 3]
    want = fs.rows_of("straddle300", lambda: fs.brute(P, 300, batch=batch, num_batches=B))
    got = check_both(eng, want, 300, starts=layout(eng))
    assert got["counts"].tolist() == [5, 40, 1, 16, 17, 300]


def test_two_level_two_boxes(eng):
    P = fs.uniform_case(70000, 712)
    eng.build(P)
    tree = eng.export_tree_ex()
    assert tree["wide_levels"] == 3 and tree["wide_count"][2] == 2
    want = fs.rows_of("uniform70000", lambda: fs.brute(P, 300))
    got = run(eng, 300)
    same(got, want)
    rule = fs.visited_blocks(tree, 300)
    assert np.array_equal(rule["idx"], want["idx"])
    assert got["info"]["point_tests"] == 16 * int(rule["visits"][0])
    assert got["info"]["point_tests"] * 2 < 16 * int(rule["touching"][0]) * 300, "the tree prunes"


def test_lattice_ties_go_to_the_smallest_name(eng):
    P = fs.lattice_case()
    eng.build(P)
    check_both(eng, fs.rows_of("lattice", lambda: fs.brute(P, 200)), 200)


def test_duplicates_come_last(eng):
    P = fs.duplicates_case()
    eng.build(P)
    got = check_both(eng, fs.rows_of("duplicates", lambda: fs.brute(P, 1024)), 1024)
    assert (got["dist"][0, 512:] == 0).all() and (np.diff(got["idx"][0, 512:]) > 0).all() and sorted(got["idx"][0]) == list(range(1024))


def test_ids_name_the_samples(eng):
    P, ids = fs.ids_case()
    eng.build(P, ids=ids)
    got = check_both(eng, fs.brute(P, 300, ids=ids), 300)
    assert got["idx"][0, 0] == ids.min() and np.isin(got["idx"][0], ids).all()


def test_planar_points(eng):
    P = fs.planar_case()
    eng.build(P)
    check_both(eng, fs.brute(P, 200), 200)


def test_nan_points_num_and_start_rows(eng):
    P, batch = fs.nan_case()
    clean = ~np.isnan(P).any(axis=1)
    sizes = [int((clean & (batch == b)).sum()) for b in range(3)]
    eng.build(P, batch=batch, num_batches=3)
    starts = layout(eng)
    assert (starts[1:] - starts[:-1]).tolist() == sizes
    got = check_both(eng, fs.brute(P, 400, batch=batch, num_batches=3), 400, starts=starts)
    assert got["counts"].tolist() == sizes and not np.isin(np.flatnonzero(~clean), got["idx"]).any()
    # d_num of 0, 1 and more than n_b
    num = np.array([0, 1, 10**6], np.int32)
    got = check_both(eng, fs.brute(P, 300, batch=batch, num_batches=3, num=num), 300, starts=starts, num=num)
    assert got["counts"].tolist() == [0, 1, min(300, sizes[2])]
    num = np.array([-5, 2**31 - 1, 3], np.int32)
    check_both(eng, fs.brute(P, 20, batch=batch, num_batches=3, num=num), 20, starts=starts, num=num)
    # start rows: valid, negative, of another cloud, of a NaN point, out of range
    own = [int(np.flatnonzero(clean & (batch == b))[7]) for b in range(3)]
    nan_row = int(np.flatnonzero(~clean & (batch == 1))[0]) if (~clean & (batch == 1)).any() else int(np.flatnonzero(~clean)[0])
    for rows, bad in (([own[0], own[1], own[2]], 0), ([-1, -7, own[2]], 0), ([own[1], own[1], own[0]], 2), ([own[0], nan_row, 800], 2),
                      ([2**31 - 1, -2**31, own[2]], 1)):
        rows = np.array(rows, np.int32)
        want = fs.brute(P, 30, batch=batch, num_batches=3, start_rows=rows)
        assert want["bad_starts"] == bad
        got = check_both(eng, want, 30, starts=starts, start_rows=rows)
        assert got["info"]["bad_starts"] == want["bad_starts"]


def test_32_clouds_of_4096(eng):
    P, batch = fs.many_clouds_case(32, 4096, 720)
    eng.build(P, batch=batch)
    seeded = [0, 13, 31]
    want = fs.rows_of("32x4096", lambda: fs.brute(P, 1024, batch=batch, num_batches=32, clouds=seeded))
    got = run(eng, 1024)
    same(got, want, seeded)
    assert (got["counts"] == 1024).all() and got["info"]["samples"] == 32 * 1024
    for b in range(32):
        assert len(np.unique(got["idx"][b])) == 1024 and (got["idx"][b] // 4096 == b).all()
    # the rule, exactly, on the seeded clouds alone
    num = np.zeros(32, np.int32)
    num[seeded] = 1024
    only = run(eng, 1024, num=num)
    same(only, want, seeded)
    rule = fs.visited_blocks(eng.export_tree_ex(), 1024, starts=layout(eng), num=num, clouds=seeded)
    assert np.array_equal(rule["idx"][seeded], want["idx"][seeded])
    assert only["info"]["point_tests"] == 16 * int(rule["visits"].sum()) and only["info"]["samples"] == 3 * 1024
    assert only["info"]["point_tests"] * 4 <= 3 * 4096 * 1024, "at most a quarter of brute force's point updates"


def test_1024_clouds_of_64(eng):
    P, batch = fs.many_clouds_case(1024, 64, 721)
    perm = np.random.default_rng(722).permutation(len(P))
    P, batch = np.ascontiguousarray(P[perm]), np.ascontiguousarray(batch[perm])
    eng.build(P, batch=batch)
    want = fs.brute(P, 16, batch=batch, num_batches=1024)
    same(run(eng, 16), want)
    same(run(eng, 16, prune=False), want)


def test_one_cloud_batched_equals_plain(eng):
    P = fs.uniform_case(5000, 730)
    eng.build(P)
    plain = run(eng, 400)
    eng.build(P, batch=np.zeros(5000, np.int32), num_batches=1)
    one = run(eng, 400)
    same(one, plain)
    assert one["info"]["point_tests"] == plain["info"]["point_tests"]
    same(plain, fs.brute(P, 400))


def test_solve_and_halo_are_left_alone(eng):
    from owlraytracing_amd import datasets

    P = fs.uniform_case(4000, 731)
    H = (fs.uniform_case(300, 732) + np.float32(1.0)).astype(np.float32)
    eng.build(P)
    eng.set_halo(H, ids=np.arange(4000, 4300, dtype=np.int32))
    k, r0 = 5, datasets.start_radius(4000, 5)
    before = eng.solve(k, r0)
    halo_before = eng.export_tree_ex(halo=True)
    tree_before = eng.export_tree_ex()
    got = run(eng, 200)
    same(got, fs.brute(P, 200))
    after = eng.solve(k, r0)
    assert np.array_equal(before["idx"].cpu().numpy(), after["idx"].cpu().numpy())
    assert np.array_equal(before["dist"].cpu().numpy().view(np.int32), after["dist"].cpu().numpy().view(np.int32))
    for name, a in halo_before.items():
        assert np.array_equal(np.asarray(a), np.asarray(eng.export_tree_ex(halo=True)[name])), name
    for name, a in tree_before.items():
        assert np.array_equal(np.asarray(a), np.asarray(eng.export_tree_ex()[name])), name
    eng.set_halo(None)


def test_front_end_and_one_shot():
    import owlraytracing_amd
    from owlraytracing_amd.trueknn import TrueKNN
    from owlraytracing_amd.trueknn import fps as one_shot

    P, batch = fs.nan_case()
    clean = ~np.isnan(P).any(axis=1)
    sizes = np.array([(clean & (batch == b)).sum() for b in range(3)])
    ratio = 0.37
    num = np.ceil(np.float64(ratio) * sizes).astype(np.int32)
    want = fs.brute(P, int(num.max()), batch=batch, num_batches=3, num=num)
    e = TrueKNN(device=0)
    e.build(P, batch=batch)
    got = e.fps(ratio=ratio)
    assert tuple(got["idx"].shape) == (3, int(num.max())) and got["counts"].cpu().numpy().tolist() == num.tolist()
    assert np.array_equal(got["idx"].cpu().numpy(), want["idx"]) and np.array_equal(got["dist"].cpu().numpy().view(np.int32), want["dist"].view(np.int32))
    assert "dist" not in e.fps(num_samples=4, want_dist=False)
    assert e.fps(num=num)["counts"].cpu().numpy().tolist() == num.tolist()
    with pytest.raises(ValueError):
        e.fps(num_samples=4, ratio=0.5)
    with pytest.raises(ValueError):
        e.fps()
    with pytest.raises(ValueError):
        e.fps(num_samples=4, start_rows=np.zeros(2, np.int32))
    # a plain tree with NaN points: ratio of the points without one
    e.build(P)
    got = e.fps(ratio=0.25)
    assert got["counts"].cpu().numpy().tolist() == [int(np.ceil(0.25 * clean.sum()))]
    e.close()
    flat = want["idx"][want["idx"] >= 0]
    for call in (one_shot, owlraytracing_amd.fps):
        rows = call(P, batch, ratio=ratio)
        assert rows.dtype == np.int64 and np.array_equal(rows, flat)
    rows = one_shot(fs.uniform_case(100, 740))
    assert len(rows) == 50 and len(np.unique(rows)) == 50 and rows[0] == 0
