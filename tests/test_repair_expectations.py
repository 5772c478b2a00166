"""CPU checks of what tests/test_repair_exact_gpu.py relies on: the sets it uses really tell an exact-kNN pass from the
rule tknnRepairExact used to follow, so that the GPU tests cannot pass for the wrong reason.

The old rule walked again only the rows whose k-th distance d_k exceeds their final box half-width r_q = r0 * 2**level,
and kept every other row of the replay (oracle.trueknn_numpy): rows whose candidates tie at bit-identical distances in the
replay's order (first level seen, then index), and, after a solve with per-query start radii, every row, since r_q was
computed from one placeholder start radius.  The rule now: walk every finished row.  A walk is a box of half-width
fl32(fl32(d_k * 1.000001) + 2**-74) around the query (the old rule had no 2**-74), its points other than the query in
(dist, index) order."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import oracle
import tile_sets
from conftest import load_golden
from oracle.trueknn_numpy import distance32, trueknn_numpy
from owlraytracing_amd import datasets


FLOOR = np.float32(2.0 ** -74)  # added to the half-width by the current rule: bounds the offsets of subnormal squares


def repair_rows(xyz, idx, dist, level, r0, walk_all, ids=None, floor=None):
    """The repair pass in numpy.  ``r0``: one start radius, or one per row; ``walk_all``: the current rule (every row with
    level >= 0, half-width fl32(fl32(d_k * 1.000001) + 2**-74)), else the old one (only rows with d_k > r_q, half-width
    fl32(d_k * 1.000001)); ``floor`` overrides the term added.  Returns (idx, dist, walked)."""
    floor = (FLOOR if walk_all else np.float32(0)) if floor is None else np.float32(floor)
    xyz = np.ascontiguousarray(xyz, np.float32)
    ids = np.arange(len(xyz)) if ids is None else np.asarray(ids)
    idx, dist = idx.copy(), dist.copy()
    k = idx.shape[1]
    r0 = np.broadcast_to(np.float32(r0), (len(xyz),))
    tree = cKDTree(xyz.astype(np.float64))
    walked = np.zeros(len(xyz), bool)
    for q in np.nonzero(level >= 0)[0]:
        dk = dist[q, k - 1]
        if not walk_all and not dk > tile_sets.halo_radius(r0[q], int(level[q])):
            continue
        walked[q] = True
        r = np.float32(np.float32(dk * np.float32(1.000001)) + floor)
        p = np.asarray(tree.query_ball_point(xyz[q].astype(np.float64), float(r) * 1.0001 + 1e-30, p=np.inf), np.int64)
        p = p[p != q]
        c = xyz[p]
        p = p[np.all(((c - r).astype(np.float32) <= xyz[q]) & (xyz[q] <= (c + r).astype(np.float32)), axis=1)]
        d = distance32(xyz[p], xyz[q])
        order = np.lexsort((ids[p], d))[:k]
        idx[q], dist[q] = -1, np.float32(3.402823466e38)  # (a box that cuts neighbours leaves empty slots)
        idx[q, : len(order)], dist[q, : len(order)] = ids[p][order], d[order]
    return idx, dist, walked


def differing_rows(idx, dist, bi, bd):
    return (idx != bi).any(axis=1) | (dist.view(np.int32) != bd.view(np.int32)).any(axis=1)


def tie_case(name, k):
    if name == "crossgolden":
        return load_golden("crossroundties_n400_k2")["xyz"], 1.0
    if name == "boundary":
        xyz, r0, _ = tile_sets.repair_boundary_case()
        return xyz, r0
    return tile_sets.tie_set(name)


# (set, k, does the old rule leave wrong rows): on the lattice and the duplicates every tie is met in one round or
# decided by the old rule's own walk; they stay in the GPU tests as exactness checks of ties.
TIE_CASES = [("crossgolden", 2, True), ("crossgolden", 3, True), ("crossgolden", 5, True), ("boundary", 2, True),
             ("quantised", 5, True), ("quantised", 16, True), ("lattice", 6, False), ("duplicates", 4, False)]


@pytest.mark.parametrize("name,k,old_wrong", TIE_CASES)
def test_tie_sets_against_the_old_and_the_new_rule(name, k, old_wrong):
    """Where marked, the old rule leaves rows that brute force orders differently -- rows it does not walk, because
    d_k <= r_q.  Walking every finished row gives brute force on every row of every set."""
    xyz, r0 = tie_case(name, k)
    rep = trueknn_numpy(xyz, k, r0)
    bi, bd = oracle.bruteforce_knn(xyz, k)
    oi, od, walked = repair_rows(xyz, rep["idx"], rep["dist"], rep["level"], r0, walk_all=False)
    wrong = differing_rows(oi, od, bi, bd)
    assert wrong.any() == old_wrong and not (wrong & walked).any()
    ni, nd, walked = repair_rows(xyz, rep["idx"], rep["dist"], rep["level"], r0, walk_all=True)
    assert walked.all()
    assert np.array_equal(ni, bi) and np.array_equal(nd.view(np.int32), bd.view(np.int32))


def test_cross_round_golden_counts():
    """On the cross-round golden set the old rule leaves 76 rows wrong at each of k = 2, 3 and 5, none of them walked;
    at k = 2, 51 of them hold another set of points than brute force."""
    xyz = load_golden("crossroundties_n400_k2")["xyz"]
    for k in (2, 3, 5):
        rep = trueknn_numpy(xyz, k, 1.0)
        bi, bd = oracle.bruteforce_knn(xyz, k)
        oi, od, walked = repair_rows(xyz, rep["idx"], rep["dist"], rep["level"], 1.0, walk_all=False)
        wrong = differing_rows(oi, od, bi, bd)
        assert wrong.sum() == 76 and not (wrong & walked).any()
        if k == 2:
            assert sum(set(a) != set(b) for a, b in zip(oi[wrong], bi[wrong])) == 51


def test_boundary_row_has_no_tie_inside_it():
    """The hand-built row: level 1, r_q = 9 >= d_k = 5, two distinct distances in the row, and still another point at
    the k-th place than brute force: a test for ties inside the row cannot find it."""
    xyz, r0, k = tile_sets.repair_boundary_case()
    rep = trueknn_numpy(xyz, k, r0)
    assert rep["level"][0] == 1 and rep["dist"][0, k - 1] == 5 and tile_sets.halo_radius(r0, 1) == 9
    assert len(set(rep["dist"][0].tolist())) == k
    assert rep["idx"][0].tolist() == [3, 2]
    bi, _ = oracle.bruteforce_knn(xyz, k)
    assert bi[0].tolist() == [3, 1]


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_per_query_radii_with_a_placeholder_walk_nothing(kind):
    """After a solve with per-query start radii, levels count doublings of each row's own radius; the old rule took r_q
    from the placeholder start radius 1.0, which is above every d_k here, and so walked no row.  Those rows are not
    exact kNN; walking every finished row makes them so."""
    n, k = 3000, 8
    rng = np.random.default_rng(11)
    if kind == "uniform":
        xyz = datasets.uniform3d(n, seed=12)
    else:
        xyz = datasets.gaussian_mixture3d(n, components=5, sigma=0.03, seed=13)
    radii = rng.choice(np.float32([0.01, 0.02, 0.05]), n).astype(np.float32)
    ref = oracle.trueknn_per_query(xyz, k, radii)
    level = np.full(n, -1, np.int32)
    for r in np.unique(radii):
        q = np.flatnonzero(radii == r)
        level[q] = trueknn_numpy(xyz, k, float(r), query_ids=q)["level"][q]
    assert (level >= 0).all()
    bi, bd = oracle.bruteforce_knn(xyz, k)
    assert differing_rows(ref["idx"], ref["dist"], bi, bd).sum() > n // 50
    _, _, walked = repair_rows(xyz, ref["idx"], ref["dist"], level, 1.0, walk_all=False)
    assert not walked.any()
    oi, od, walked = repair_rows(xyz, ref["idx"], ref["dist"], level, radii, walk_all=False)
    assert walked.any()  # (with each row's own radius the old rule would have walked some)
    ni, nd, _ = repair_rows(xyz, ref["idx"], ref["dist"], level, 1.0, walk_all=True)
    assert np.array_equal(ni, bi) and np.array_equal(nd.view(np.int32), bd.view(np.int32))


@pytest.mark.parametrize("scale", [1.0, 1e-6, 1e-12, 1e-18, 1e-21, 1e-24])
def test_magnitudes(scale):
    """Uniform points scaled down to where squared offsets are subnormal (1e-21) or vanish (1e-24).  With d_k * 1.000001
    alone the box cuts true neighbours there: sqrt of a subnormal keeps few bits.  Adding 2**-74, above the square root of
    the largest error of three subnormal squares, keeps every point of computed distance <= d_k in the box."""
    xyz = (datasets.uniform3d(1500, seed=21) * np.float32(scale)).astype(np.float32)
    k = 6
    r0 = np.float32(datasets.start_radius(len(xyz), k) * scale)
    rep = trueknn_numpy(xyz, k, r0)
    bi, bd = oracle.bruteforce_knn(xyz, k)
    ni, nd, _ = repair_rows(xyz, rep["idx"], rep["dist"], rep["level"], r0, walk_all=True)
    assert np.array_equal(ni, bi) and np.array_equal(nd.view(np.int32), bd.view(np.int32))
    ci, cd, _ = repair_rows(xyz, rep["idx"], rep["dist"], rep["level"], r0, walk_all=True, floor=0)
    assert differing_rows(ci, cd, bi, bd).any() == (scale < 1e-18)
