"""TrueKNN.match_features (tknnFeatureMatch, include/owlknn_global.h) against its numpy definition (tests/global_spec.py), bit for
bit: the best row, its squared distance and the second-best squared distance -- at widths on both sides of the padding to a
multiple of four and of the two register tiles, across chunk edges, with ties, duplicates, rows that are not finite, and no rows."""
import contextlib
import os

import numpy as np
import pytest

import global_spec as gs

pytestmark = pytest.mark.gpu

CHUNK = "TKNN_MATCH_CHUNK"


@contextlib.contextmanager
def chunk(rows):
    before = os.environ.pop(CHUNK, None)
    if rows:
        os.environ[CHUNK] = str(rows)
    try:
        yield
    finally:
        os.environ.pop(CHUNK, None)
        if before is not None:
            os.environ[CHUNK] = before


@pytest.fixture(scope="module")
def eng():
    from owlraytracing_amd.trueknn import TrueKNN

    e = TrueKNN(device=0)  # no tree: the call needs none
    yield e
    e.close()


def run(eng, A, B, **kw):
    r = eng.match_features(np.asarray(A, np.float32), np.asarray(B, np.float32), **kw)
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


def bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def check(r, A, B, what=""):
    best, b1, b2 = gs.match(A, B)
    assert np.array_equal(r["best"], best), what + ": best"
    assert np.array_equal(bits(r["best_d2"]), bits(b1)), what + ": best_d2"
    assert np.array_equal(bits(r["second_d2"]), bits(b2)), what + ": second_d2"
    assert np.array_equal(r["pairs"], gs.filter_pairs(best, b1, b2)), what + ": pairs"
    return best, b1, b2


def rows(rng, count, D):
    return (rng.random((count, D)) * 4 - 2).astype(np.float32)


@pytest.mark.parametrize("m,n,D", [(257, 130, 33), (64, 65, 1), (70, 300, 4), (70, 300, 5), (33, 200, 64), (5, 1, 33)])
def test_shapes(eng, m, n, D):
    rng = np.random.default_rng(100 * D + n)
    A, B = rows(rng, m, D), rows(rng, n, D)
    r = run(eng, A, B)
    _, _, b2 = check(r, A, B, "(%d, %d, %d)" % (m, n, D))
    assert r["info"]["pair_tests"] == m * n and r["info"]["bad_source_rows"] == 0 and r["info"]["bad_target_rows"] == 0 and r["info"]["chunks"] >= 1
    assert np.isinf(b2).all() == (n == 1)


def test_ties_and_duplicates(eng):
    """Exact duplicates in the target (second == best, the smaller row wins) and planted equal distances of different rows."""
    rng = np.random.default_rng(1)
    B = rng.integers(-3, 4, size=(90, 6)).astype(np.float32)  # small integers: every distance is exact, ties abound
    B[40] = B[7]
    B[80] = B[7]
    A = np.concatenate([B[[7, 80, 40, 3]], rng.integers(-3, 4, size=(60, 6)).astype(np.float32)])
    A[5] = 0
    B[10], B[20] = 0, 0
    B[10, 0], B[20, 1] = 2, -2  # both at distance 4 of A[5]
    r = run(eng, A, B)
    best, b1, b2 = check(r, A, B)
    assert best[0] == 7 and best[1] == 7 and best[2] == 7 and b1[0] == 0 and b2[0] == 0
    assert (b1 == b2).sum() >= 10, "the case has ties"
    with chunk(16):
        check(run(eng, A, B), A, B, "chunks of 16")


def test_rows_that_are_not_finite(eng):
    rng = np.random.default_rng(2)
    A, B = rows(rng, 140, 33), rows(rng, 150, 33)
    A[3, 0], A[77, 32], A[139, 5] = np.nan, np.inf, -np.inf
    B[0, 1], B[64, 0], B[149, 32], B[100, 7] = np.nan, np.inf, -np.inf, np.nan
    r = run(eng, A, B)
    best, b1, b2 = check(r, A, B)
    assert (best[[3, 77, 139]] == -1).all() and np.isinf(b1[[3, 77, 139]]).all() and not np.isin(best, [0, 64, 149, 100]).any()
    assert r["info"]["bad_source_rows"] == 3 and r["info"]["bad_target_rows"] == 4 and r["info"]["pair_tests"] == 137 * 146
    # every target row left out: nobody has a match
    r = run(eng, A[:9], np.full((5, 33), np.nan, np.float32))
    assert (r["best"] == -1).all() and np.isinf(r["best_d2"]).all() and np.isinf(r["second_d2"]).all() and len(r["pairs"]) == 0
    # distances that overflow to +inf are distances still: the smaller row
    big = np.float32([[3e38, -3e38]])
    r = run(eng, big, -np.repeat(big, 3, axis=0))
    check(r, big, -np.repeat(big, 3, axis=0))
    assert r["best"][0] == 0 and np.isinf(r["best_d2"][0]) and np.isinf(r["second_d2"][0])


def test_no_rows(eng):
    rng = np.random.default_rng(3)
    r = run(eng, np.zeros((0, 33), np.float32), rows(rng, 10, 33))
    assert r["best"].shape == (0,) and r["pairs"].shape == (0, 2) and r["info"]["pair_tests"] == 0 and r["info"]["chunks"] == 0 and r["info"]["solve_ms"] == 0
    r = run(eng, rows(rng, 70, 33), np.zeros((0, 33), np.float32))
    assert (r["best"] == -1).all() and np.isinf(r["best_d2"]).all() and np.isinf(r["second_d2"]).all() and r["pairs"].shape == (0, 2)
    assert r["info"]["chunks"] == 0 and r["info"]["pair_tests"] == 0


@pytest.mark.parametrize("n", [130, 129])
def test_chunk_edges(eng, n):
    """Chunks of 64 rows: the last has 2 rows or 1.  The best and the second of some rows are planted on both sides of an edge."""
    rng = np.random.default_rng(n)
    A, B = rows(rng, 200, 33), rows(rng, n, 33)
    B[63], B[64], B[n - 1] = A[0], A[0], A[1]
    B[64, 0] += np.float32(0.5)
    B[127] = A[1]
    B[127, 3] -= np.float32(0.25)
    plain = run(eng, A, B)
    with chunk(64):
        forced = run(eng, A, B)
    with chunk(1000):
        whole = run(eng, A, B)
    best, _, _ = check(forced, A, B, "chunks of 64")
    assert forced["info"]["chunks"] == 3 and whole["info"]["chunks"] == 1
    assert best[0] == 63 and best[1] == n - 1
    for other in (plain, whole):
        for name in ("best", "best_d2", "second_d2"):
            assert np.array_equal(forced[name].view(np.int32), other[name].view(np.int32)), name


def test_fpfh_like_rows_and_two_runs(eng):
    rng = np.random.default_rng(4)
    A, B = gs.fpfh_like(rng, 300), gs.fpfh_like(rng, 520)
    B[100] = A[5]
    first = run(eng, A, B)
    best, b1, _ = check(first, A, B)
    assert best[5] == 100 and b1[5] == 0
    again = run(eng, A, B)
    for name in ("best", "best_d2", "second_d2"):
        assert np.array_equal(first[name].view(np.int32), again[name].view(np.int32)), name
    with chunk(64):
        check(run(eng, A, B), A, B, "chunks of 64")


def test_four_rows_per_lane(eng):
    """The register tile that was measured and not adopted (TKNN_MATCH_ROWS=4, up to 36 channels) gives the same bits."""
    before = os.environ.pop("TKNN_MATCH_ROWS", None)
    os.environ["TKNN_MATCH_ROWS"] = "4"
    try:
        for m, n, D in ((1100, 130, 33), (70, 300, 4), (33, 200, 64)):
            rng = np.random.default_rng(D)
            A, B = rows(rng, m, D), rows(rng, n, D)
            with chunk(64):
                check(run(eng, A, B), A, B, "four rows per lane, (%d, %d, %d)" % (m, n, D))
    finally:
        os.environ.pop("TKNN_MATCH_ROWS", None)
        if before is not None:
            os.environ["TKNN_MATCH_ROWS"] = before


def test_mutual_and_ratio_filters(eng):
    rng = np.random.default_rng(5)
    B = gs.fpfh_like(rng, 260)
    A = (B[rng.permutation(260)[:180]] + rng.normal(scale=0.5, size=(180, 33)).astype(np.float32)).astype(np.float32)
    A = np.concatenate([A, gs.fpfh_like(rng, 40)])
    A[7, 2] = np.nan
    s_best, s1, s2 = gs.match(A, B)
    t_best, _, _ = gs.match(B, A)
    for mutual, ratio in ((True, 0.9), (True, None), (False, 0.9), (False, 0.5)):
        want = gs.filter_pairs(s_best, s1, s2, t_best if mutual else None, ratio)
        r = run(eng, A, B, mutual=mutual, ratio=ratio, want_dist=True)
        assert np.array_equal(r["pairs"], want), (mutual, ratio)
        assert np.array_equal(bits(r["dist"]), bits(np.sqrt(s1[want[:, 0]])))
        assert 0 < len(want) < len(A)
    from owlraytracing_amd.trueknn import match_features

    # no target rows, or no source rows: no pairs, with and without the filters
    for mutual, ratio in ((True, 0.9), (True, None), (False, None)):
        r = run(eng, A, np.zeros((0, 33), np.float32), mutual=mutual, ratio=ratio)
        assert r["pairs"].shape == (0, 2) and (r["best"] == -1).all()
        assert run(eng, np.zeros((0, 33), np.float32), B, mutual=mutual, ratio=ratio)["pairs"].shape == (0, 2)
    one = match_features(A, B, mutual=True, ratio=0.9)
    assert np.array_equal(one["pairs"], gs.filter_pairs(s_best, s1, s2, t_best, 0.9))
