"""What TrueKNN.query (tknnQuery) must return, restated in numpy, and the point sets its tests run on.  No tests here.

Row j is the row the reference's loop gives to q_j in the set P + {q_j}, q_j being the query there:
  * level L uses the radius r_L = start radius doubled L times in float32;
  * the candidates of level L are the points p of P with fl(p - r_L) <= q_j <= fl(p + r_L) on every axis;
  * the query finishes at the first level with at least k candidates; its row is the k smallest
    (distance, level at which the candidate first was one, index) triples -- index = id where ids are given;
  * intersections = candidates summed over the levels traced; levels = that level, -1 if max_rounds levels did not do;
  * nothing is "self": a point of P that coincides with q_j is a neighbour at distance 0.
The yardstick for these values is oracle.trueknn_rows(concat(P, q_j), k, r, query_ids=[n]), one call per query
(tests/test_query_expectations.py holds the two against each other); this file is what the GPU tests compare with,
every row of every set.  Candidates are proposed by a Chebyshev ball query with a margin; the fp32 box test decides.
"""
import numpy as np
from scipy.spatial import cKDTree

from owlraytracing_amd import datasets
from owlraytracing_amd.datasets import pad_to_3d

import tile_sets


def distance32(c, q):
    """sqrt((dx*dx + dy*dy) + dz*dz), every operation rounded to float32 (as oracle/trueknn_numpy.py::distance32)."""
    d = c.astype(np.float32) - q.astype(np.float32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.sqrt(((x * x) + (y * y)) + (z * z), dtype=np.float32)


def in_box(P, q, r):
    r = np.float32(r)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.all((P - r <= q) & (q <= P + r), axis=1)


def query_rows(P, Q, ks, start_radius, ids=None, max_rounds=64):
    """{k: dict(idx (m,k) int32, dist (m,k) float32, intersections (m,) int64, levels (m,) int32, rounds,
    final_radius, total_intersections, total_active_rounds, unfinished)} for every k of ``ks`` in one pass over the
    queries.  Rows of unfinished queries hold -1 / nan and intersections 0: the engine does not write them."""
    P, Q = pad_to_3d(np.asarray(P, np.float32)), pad_to_3d(np.asarray(Q, np.float32))
    n, m = len(P), len(Q)
    ks = sorted(set(int(k) for k in ks))
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    clean = ~np.isnan(P).any(axis=1)
    tree = cKDTree(P[clean].astype(np.float64))
    clean_pos = np.flatnonzero(clean)
    out = {k: {"idx": np.full((m, k), -1, np.int32), "dist": np.full((m, k), np.nan, np.float32),
               "intersections": np.zeros(m, np.int64), "levels": np.full(m, -1, np.int32), "traced": np.zeros(m, np.int64)}
           for k in ks}
    for j in range(m):
        q = Q[j]
        todo = list(ks)
        r = np.float32(start_radius)
        isect = 0
        prev_c = np.zeros(0, np.int64)
        prev_first = np.zeros(0, np.int64)
        level = 0
        while todo and level < max_rounds:
            if np.isnan(q).any():
                c = np.zeros(0, np.int64)
            elif not np.isfinite(r) or float(r) > 1e30:
                c = clean_pos
            else:
                reach = float(r) * 1.0001 + 1e-5 * (float(np.abs(q).max()) + float(r)) + 1e-30
                c = clean_pos[np.sort(np.asarray(tree.query_ball_point(q.astype(np.float64), reach, p=np.inf), np.int64))]
            if len(c):
                c = c[in_box(P[c], q, r)]
            first = np.full(len(c), level, np.int64)
            if len(prev_c) and len(c):
                pos = np.clip(np.searchsorted(prev_c, c), 0, len(prev_c) - 1)
                seen = prev_c[pos] == c
                first[seen] = prev_first[pos[seen]]
            prev_c, prev_first = c, first
            isect += len(c)
            if len(c) >= todo[0]:
                d = distance32(P[c], q)
                order = np.lexsort((ids[c], first, d))
                while todo and len(c) >= todo[0]:
                    k = todo.pop(0)
                    o = out[k]
                    o["idx"][j] = ids[c[order[:k]]]
                    o["dist"][j] = d[order[:k]]
                    o["intersections"][j] = isect
                    o["levels"][j] = level
                    o["traced"][j] = level + 1
            level += 1
            r = np.float32(r * np.float32(2))
        for k in todo:
            out[k]["traced"][j] = max_rounds
    for k in ks:
        o = out[k]
        fin = o["levels"] >= 0
        o["unfinished"] = int((~fin).sum())
        o["rounds"] = int(o["traced"].max()) if m else 0
        radius = np.float32(start_radius)
        for _ in range(1, o["rounds"]):
            radius = np.float32(radius * np.float32(2))
        o["final_radius"] = float(radius)
        o["total_intersections"] = int(o["intersections"][fin].sum())
        o["total_active_rounds"] = int(o["traced"].sum())
    return out


def exact_rows(P, Q, k, ids=None):
    """The true k nearest points of P to every query in (dist, index) order with the fp32 distance formula: brute force."""
    P, Q = pad_to_3d(np.asarray(P, np.float32)), pad_to_3d(np.asarray(Q, np.float32))
    ids = np.arange(len(P), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    idx = np.empty((len(Q), k), np.int32)
    dist = np.empty((len(Q), k), np.float32)
    for j in range(len(Q)):
        d = distance32(P, Q[j])
        order = np.lexsort((ids, d))[:k]
        idx[j] = ids[order]
        dist[j] = d[order]
    return idx, dist


def lattice_queries(P, count, seed, step=np.float32(1.0 / 32)):
    """A third each: lattice nodes (points of P itself), cell centres, edge midpoints -- rows full of bit-identical distances."""
    rng = np.random.default_rng(seed)
    third = count // 3
    nodes = P[rng.choice(len(P), third, replace=False)]
    centres = P[rng.choice(len(P), third, replace=False)] + step / 2
    mids = P[rng.choice(len(P), count - 2 * third, replace=False)].copy()
    mids[np.arange(len(mids)), rng.integers(0, 3, len(mids))] += step / 2
    return np.ascontiguousarray(np.concatenate([nodes, centres, mids]).astype(np.float32))


SET_NAMES = ("uniform", "copies", "lattice", "duplicates", "planar", "clustered", "tiny", "scale_down", "scale_up")
N_WIDE = 500  # the last queries of the uniform set: a cube twice as wide as the tree's


def make_set(name):
    """(P, Q, r0) of a named set; every set has queries chosen to hit one behaviour (see the table in the test files)."""
    if name in ("uniform", "copies"):
        P = datasets.uniform3d(20000, seed=31)
        if name == "copies":
            rng = np.random.default_rng(32)
            return P, np.ascontiguousarray(P[rng.permutation(len(P))[:2000]]), 0.01
        rng = np.random.default_rng(33)
        inside = rng.random((5000, 3), dtype=np.float32)
        wide = rng.random((N_WIDE, 3), dtype=np.float32) * np.float32(2) - np.float32(0.5)
        return P, np.concatenate([inside, wide]), 0.01
    if name == "lattice":
        P = tile_sets.lattice(12, 3, 1)
        return P, lattice_queries(P, 600, 2), float(np.float32(0.3 / 32))
    if name == "duplicates":
        P = tile_sets.with_duplicates(4000, 4)
        rng = np.random.default_rng(34)
        rep = P[rng.integers(0, len(P), 500)]
        return P, np.concatenate([rng.random((1000, 3), dtype=np.float32), rep]), 0.03
    if name == "planar":
        rng = np.random.default_rng(35)
        P = pad_to_3d(rng.random((4000, 2), dtype=np.float32))
        flat = pad_to_3d(rng.random((800, 2), dtype=np.float32))
        off = rng.random((400, 3), dtype=np.float32) * np.float32([1, 1, 0.1])
        return P, np.concatenate([flat, off]), 0.01
    if name == "clustered":
        P = datasets.gaussian_mixture3d(20000, components=64, sigma=0.005, seed=5)
        rng = np.random.default_rng(36)
        lo, hi = P.min(0), P.max(0)
        return P, (lo + rng.random((1500, 3), dtype=np.float32) * (hi - lo)).astype(np.float32), 0.004
    if name == "tiny":
        rng = np.random.default_rng(37)
        return rng.random((5, 3), dtype=np.float32), rng.random((3, 3), dtype=np.float32), 0.05
    if name in ("scale_down", "scale_up"):
        s = np.float32(1e-6 if name == "scale_down" else 1e6)
        rng = np.random.default_rng(38)
        P = ((datasets.uniform3d(4000, seed=39) + np.float32(1e3)) * s).astype(np.float32)
        Q = ((rng.random((800, 3), dtype=np.float32) + np.float32(1e3)) * s).astype(np.float32)
        return P, Q, float(np.float32(0.02) * s)
    raise KeyError(name)


ALL_K = (1, 2, 5, 10, 16, 17, 32, 33, 64)  # every register capacity and the full lists k = 16 * NREG


def ks_for(name, ks=ALL_K):
    n = 5 if name == "tiny" else 10 ** 9
    return tuple(k for k in ks if k <= n)
