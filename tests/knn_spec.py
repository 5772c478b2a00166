"""What TrueKNN.knn (tknnKnn) must return, restated in numpy, and the cases its tests share.  No tests here.

Row j holds the k nearest points of the built set P to q_j.  Brute force over every pair, no tree and no radius:
  * the distance is the fp32 formula sqrt((dx*dx + dy*dy) + dz*dz), every operation rounded to float32;
  * only points at a FINITE distance are eligible: a NaN coordinate on either side makes the distance NaN (a NaN query has an
    empty row, NaN points of P are nobody's neighbour), a distance that overflows is not a neighbour's either;
  * the point skip[j] names (a negative value: none) is not eligible; in self mode (the queries are P's own points) skip[j] is
    point j itself -- by its id where ids are given --, while a coinciding duplicate stays, at distance 0;
  * the eligible points in stable (distance, index) order -- index = id where ids are given --, cut after k, padded with idx -1 /
    dist +inf; counts[j] = min(k, eligible points).
"""
import numpy as np

from owlraytracing_amd.datasets import pad_to_3d

K_MAX = 64  # TKNN_MAX_K_REGISTERS


def knn_rows(P, Q, k, skip=None, ids=None, block=128):
    """dict(idx (m,k) int32, dist (m,k) float32, counts (m,) int32) of the queries Q against P."""
    P, Q = pad_to_3d(np.asarray(P, np.float32)), pad_to_3d(np.asarray(Q, np.float32))
    n, m = len(P), len(Q)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    skip = np.full(m, -1, np.int64) if skip is None else np.asarray(skip, np.int64)
    idx = np.full((m, k), -1, np.int32)
    dist = np.full((m, k), np.inf, np.float32)
    counts = np.zeros(m, np.int32)
    for s in range(0, m, block):
        with np.errstate(invalid="ignore", over="ignore"):
            d = P[None, :, :] - Q[s:s + block, None, :]  # float32 - float32
            x, y, z = d[..., 0], d[..., 1], d[..., 2]
            d = np.sqrt(((x * x) + (y * y)) + (z * z), dtype=np.float32)
        assert d.dtype == np.float32
        for t in range(d.shape[0]):
            j = s + t
            c = np.flatnonzero(np.isfinite(d[t]) & ((ids != skip[j]) | (skip[j] < 0)))
            if len(c) > k:  # (only what lies no farther than the k-th smallest distance can be in the row: less to sort)
                c = c[d[t, c] <= np.partition(d[t, c], k - 1)[k - 1]]
            o = c[np.lexsort((ids[c], d[t, c]))][:k]  # by distance, then by index
            counts[j] = len(o)
            idx[j, :len(o)] = ids[o]
            dist[j, :len(o)] = d[t, o]
    return {"idx": idx, "dist": dist, "counts": counts}


def self_rows(P, k, ids=None):
    """The rows of P's own points: every point left out of its own row, by its id or row."""
    return knn_rows(P, P, k, skip=np.arange(len(P)) if ids is None else ids, ids=ids)


def cut(rows, k):
    """The rows of k entries from rows of at least k (a row is the head of every longer one)."""
    assert rows["idx"].shape[1] >= k
    return {"idx": np.ascontiguousarray(rows["idx"][:, :k]), "dist": np.ascontiguousarray(rows["dist"][:, :k]),
            "counts": np.minimum(rows["counts"], k).astype(np.int32)}


_cache = {}


def rows_of(key, make):
    """The spec's rows of a named case, computed once and shared (do not write to them)."""
    if key not in _cache:
        rows = make()
        for a in rows.values():
            a.setflags(write=False)
        _cache[key] = rows
    return _cache[key]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
SET_NAMES = ("uniform", "copies", "duplicates", "planar", "scale_down", "scale_up")  # of radius_knn_spec.knn_set


def set_rows(name):
    """(P, Q, the rows of K_MAX) of a set's external queries, computed once."""
    import radius_knn_spec as rk

    P, Q, _ = rk.knn_set(name)
    return P, Q, rows_of(("set", name), lambda: knn_rows(P, Q, K_MAX))


def set_self_rows(name):
    """(P, the rows of K_MAX) of a set's own points, computed once."""
    import radius_knn_spec as rk

    P = rk.knn_set(name)[0]
    return P, rows_of(("self", name), lambda: self_rows(P, K_MAX))


def lattice_case():
    """(P, Q): the lattice of spacing 1/32 and its node / cell-centre / edge-midpoint queries -- ties at the k-th place at every
    k of radius_knn_spec.LATTICE_K, the index decides."""
    import radius_spec as rs

    return rs.lattice_case()[:2]


DUPLICATE_COPIES = 70
DUPLICATE_K = (1, 16, 64)  # the k-th distance is 0 at each: the seed bound is 0


def duplicates_case():
    """(P, Q): 1 000 uniform points of which DUPLICATE_COPIES, spread over the rows, are one point; Q[0] is that point, the other
    queries are ordinary ones."""
    from owlraytracing_amd import datasets

    P = datasets.uniform3d(1000, seed=71)
    rng = np.random.default_rng(72)
    P[rng.choice(len(P), DUPLICATE_COPIES, replace=False)] = np.float32([0.31, 0.62, 0.47])
    Q = np.concatenate([np.float32([[0.31, 0.62, 0.47]]), rng.random((15, 3), dtype=np.float32)])
    return P, np.ascontiguousarray(Q)


TINY_N = (1, 2, 16, 17, 65)


def tiny_case(n):
    """(P, Q, ks): n points, themselves and 12 others as queries, k below, equal to and above the number of points."""
    rng = np.random.default_rng(73 + n)
    P = rng.random((n, 3), dtype=np.float32)
    Q = np.concatenate([P[:40], rng.random((12, 3), dtype=np.float32) * np.float32(3) - np.float32(1)])
    ks = sorted({1, max(n - 1, 1), min(n, K_MAX), min(n + 1, K_MAX), min(n + 5, K_MAX), K_MAX})
    return P, np.ascontiguousarray(Q), ks


def nan_case():
    """(P, Q): 700 uniform points of which 23 have a NaN in one, two or three coordinates; 64 queries of which 5 have one."""
    rng = np.random.default_rng(74)
    P = rng.random((700, 3), dtype=np.float32)
    for t, row in enumerate(rng.choice(len(P), 23, replace=False)):
        P[row, : 1 + t % 3] = np.nan
    Q = rng.random((64, 3), dtype=np.float32)
    for t, row in enumerate((3, 17, 18, 40, 63)):
        Q[row, t % 3] = np.nan
    return P, Q


def far_case():
    """(P, Q): two clusters of 1 000 points 0.8 apart inside the unit cube; queries ten scene widths outside the box on every
    side and diagonal, at the midpoint between the clusters (and near it), and inside each cluster."""
    rng = np.random.default_rng(75)
    a = np.float32([0.1, 0.1, 0.1]) + rng.random((1000, 3), dtype=np.float32) * np.float32(0.05)
    b = np.float32([0.9, 0.9, 0.9]) - rng.random((1000, 3), dtype=np.float32) * np.float32(0.05)
    P = np.concatenate([a, b])
    rng.shuffle(P)
    lo, hi = P.min(0), P.max(0)
    width = float((hi - lo).max())
    away = np.float32([[s * 10 * width if axis == t else 0 for axis in range(3)] for t in range(3) for s in (-1, 1)])
    mid = (lo + hi) / np.float32(2)
    Q = np.concatenate([mid + away, [mid + np.float32(10 * width)], [mid - np.float32(10 * width)], [mid], mid + (rng.random((20, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(0.01),
                        a[:10] + np.float32(0.001), b[:10] - np.float32(0.001)])
    return np.ascontiguousarray(P), np.ascontiguousarray(Q.astype(np.float32))
