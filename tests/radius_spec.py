"""What TrueKNN.radius_query (tknnRadiusQuery) must return, restated in numpy, and the cases its tests share.  No tests here.

Row j holds the points p of the built set P with dist(p, q_j) <= r, dist the fp32 formula sqrt((dx*dx + dy*dy) + dz*dz)
(query_spec.distance32):
  * distance exactly r is inside; nothing is "self": a point of P that coincides with q_j is a neighbour at distance 0;
  * a NaN coordinate on either side makes the distance NaN, which is not <= r: a NaN query has an empty row, NaN points of P
    are nobody's neighbour;
  * an entry is the point's id where ids are given, its row otherwise; with sort = 1 a row ascends in (fp32 distance, index).
Brute force: every pair's distance is computed, no kd-tree proposes candidates, so the spec cannot share a mistake with a
traversal.
"""
import numpy as np

from owlraytracing_amd.datasets import pad_to_3d

import query_spec as qs
import tile_sets
from query_spec import distance32


def radius_rows(P, Q, r, ids=None, block=256):
    """dict(offsets (m+1,) int64, idx (total,) int32, dist (total,) float32, lengths (m,) int64): the rows of the queries Q
    against P in CSR form, every row in (distance, index) order -- lexsort((ids, d))."""
    P, Q = pad_to_3d(np.asarray(P, np.float32)), pad_to_3d(np.asarray(Q, np.float32))
    n, m = len(P), len(Q)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    r = np.float32(r)
    lengths = np.zeros(m, np.int64)
    idx_rows, dist_rows = [], []
    for s in range(0, m, block):
        with np.errstate(invalid="ignore", over="ignore"):
            d = distance32(P[None, :, :], Q[s:s + block, None, :])
            near = d <= r  # (NaN <= r is False)
        for j in range(near.shape[0]):
            c = np.flatnonzero(near[j])
            dj = d[j, c]
            o = np.lexsort((ids[c], dj))
            idx_rows.append(ids[c[o]].astype(np.int32))
            dist_rows.append(dj[o].astype(np.float32))
            lengths[s + j] = len(c)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    idx = np.concatenate(idx_rows) if idx_rows else np.zeros(0, np.int32)
    dist = np.concatenate(dist_rows) if dist_rows else np.zeros(0, np.float32)
    return {"offsets": offsets, "idx": idx.astype(np.int32), "dist": dist.astype(np.float32), "lengths": lengths}


SET_NAMES = ("uniform", "copies", "duplicates", "planar", "clustered", "tiny", "scale_down", "scale_up")  # of query_spec.make_set
SET_FACTORS = (1, 3)  # r = the set's r0 times these

LATTICE_STEP = np.float32(1.0 / 32)


def lattice_case():
    """(P, Q, radii): the lattice of spacing 1/32 and its node / cell-centre / edge-midpoint queries; radii: exactly the spacing
    (neighbours at distance exactly r are in), the float below it (they are out), and half a cell's diagonal."""
    P = tile_sets.lattice(12, 3, 1)
    Q = qs.lattice_queries(P, 600, 2)
    r = LATTICE_STEP
    return P, Q, (r, np.nextafter(r, np.float32(0)), np.float32(np.sqrt(3.0) / 64.0))


CHUNK_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65)


def chunk_case():
    """(P, Q, picks): 4 096 uniform points, 64 queries, and per wanted row length L a (query, radius) pair whose row has exactly L
    entries at that radius -- the radius is the query's L-th smallest distance (for L = 0: the float below its smallest)."""
    from owlraytracing_amd import datasets

    P = datasets.uniform3d(4096, seed=51)
    Q = np.random.default_rng(52).random((64, 3), dtype=np.float32)
    picks = []
    for t, L in enumerate(CHUNK_LENGTHS):
        j = 7 * t + 3
        d = np.sort(distance32(P, Q[j]))
        r = np.nextafter(d[0], np.float32(0)) if L == 0 else d[L - 1]
        assert r > 0 and (L == 0 or d[L] > d[L - 1]), "the pick's radius must separate L from L + 1 neighbours"
        picks.append((L, j, np.float32(r)))
    return P, Q, picks


_cache = {}


def rows_of(key, make):
    """The spec's rows of a named case, computed once and shared (do not write to them)."""
    if key not in _cache:
        rows = make()
        for a in rows.values():
            a.setflags(write=False)
        _cache[key] = rows
    return _cache[key]
