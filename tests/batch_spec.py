"""What TrueKNN.batch_knn (tknnBatchKnn) and the batched build must give, restated in numpy, and the cases their tests share.
No tests here.

Row j holds the at most k nearest points of the built set P to q_j AMONG THE POINTS THAT CARRY q_j's LABEL.  Brute force over every
pair, no tree:
  * the distance is tests/knn_spec.py's: the fp32 formula sqrt((dx*dx + dy*dy) + dz*dz), every operation rounded to float32;
  * eligible are the points p with batch_p[p] == batch_q[j] at a FINITE distance (a NaN on either side: none) that is <= r_j where
    a radius is given (one for all rows, or radii[j]: a NaN, non-finite or <= 0 entry gives an empty row), except the point
    skip[j] names (a negative value: none);
  * a query whose label is outside [0, B) has an empty row (no point carries such a label);
  * in self mode the queries are P's own points with their own labels, skip[j] is point j itself -- by its id where ids are
    given --, while a coinciding duplicate of the same batch stays, at distance 0;
  * the eligible points in stable (distance, index) order -- index = id where ids are given --, cut after k, padded with idx -1 /
    dist +inf; counts[j] = min(k, eligible points).

The batched key: ((label << (63 - bb)) | (key21 >> bb)) for a point without a NaN, bit 63 alone for one with, bb = key_bits(B).
"""
import numpy as np

from owlraytracing_amd.datasets import pad_to_3d

K_MAX = 64  # TKNN_MAX_K_REGISTERS
MAX_BATCHES = 32768  # TKNN_MAX_BATCHES


def key_bits(num_batches):
    """The smallest multiple of 3 with 2**bits >= num_batches."""
    bits = 0
    while 2 ** bits < num_batches:
        bits += 3
    return bits


def batched_keys(key21, labels, num_batches):
    """The tree's keys of points whose plain 21-level keys are ``key21`` (uint64, bit 63 for a NaN point) under ``labels``."""
    bb = np.uint64(key_bits(num_batches))
    key21 = np.asarray(key21, np.uint64)
    nan = (key21 >> np.uint64(63)) != 0
    keys = (np.asarray(labels).astype(np.uint64) << (np.uint64(63) - bb)) | (key21 >> bb)
    return np.where(nan, key21, keys)


def knn_rows(P, batch_p, Q, batch_q, k, radius=None, radii=None, skip=None, ids=None, block=128):
    """dict(idx (m,k) int32, dist (m,k) float32, counts (m,) int32) of the labelled queries Q against the labelled set P."""
    P, Q = pad_to_3d(np.asarray(P, np.float32)), pad_to_3d(np.asarray(Q, np.float32))
    batch_p, batch_q = np.asarray(batch_p, np.int64), np.asarray(batch_q, np.int64)
    n, m = len(P), len(Q)
    assert batch_p.shape == (n,) and batch_q.shape == (m,)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    skip = np.full(m, -1, np.int64) if skip is None else np.asarray(skip, np.int64)
    if radii is None:
        radii = np.full(m, np.finfo(np.float32).max if radius is None else radius, np.float32)
    radii = np.asarray(radii, np.float32)
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
            r = radii[j]
            if not (np.isfinite(r) and r > 0):
                continue
            with np.errstate(invalid="ignore"):
                ok = np.isfinite(d[t]) & (d[t] <= r) & (batch_p == batch_q[j]) & ((ids != skip[j]) | (skip[j] < 0))
            c = np.flatnonzero(ok)
            o = c[np.lexsort((ids[c], d[t, c]))][:k]  # by distance, then by index
            counts[j] = len(o)
            idx[j, :len(o)] = ids[o]
            dist[j, :len(o)] = d[t, o]
    return {"idx": idx, "dist": dist, "counts": counts}


def self_rows(P, batch_p, k, ids=None, **kw):
    """The rows of P's own points in their own batches: every point left out of its own row, by its id or row."""
    return knn_rows(P, batch_p, P, batch_p, k, skip=np.arange(len(P)) if ids is None else ids, ids=ids, **kw)


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
CLOUD_SIZES = (0, 1, 5, 40, 454, 1000, 1500)  # seven clouds, each uniform in the same unit cube: n = 3000


def clouds_case():
    """(P, batch, Q, batch_q): the seven overlapping unit-cube clouds of CLOUD_SIZES with their rows shuffled, and 210 queries,
    30 per label (the empty one included), uniform in a slightly larger cube."""
    rng = np.random.default_rng(301)
    batch = np.repeat(np.arange(len(CLOUD_SIZES)), CLOUD_SIZES).astype(np.int32)
    P = rng.random((len(batch), 3), dtype=np.float32)
    perm = rng.permutation(len(batch))
    P, batch = np.ascontiguousarray(P[perm]), np.ascontiguousarray(batch[perm])
    Q = (rng.random((210, 3), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)
    batch_q = (np.arange(210) % len(CLOUD_SIZES)).astype(np.int32)
    return P, batch, Q, batch_q


def build_case(num_batches):
    """(P, batch): 3000 uniform points with unsorted random labels in [0, num_batches), one batch (label 2) left empty, and
    nine points with a NaN in one, two or three coordinates."""
    rng = np.random.default_rng(310 + num_batches)
    P = rng.random((3000, 3), dtype=np.float32)
    batch = rng.integers(0, num_batches, 3000).astype(np.int32)
    batch[batch == 2] = 3
    for t, row in enumerate(rng.choice(3000, 9, replace=False)):
        P[row, : 1 + t % 3] = np.nan
    return P, batch


def large_case(num_batches):
    """(P, batch, Q, batch_q): 20 000 uniform points with random labels, 256 queries of which a few have labels outside
    [0, num_batches) or a NaN."""
    rng = np.random.default_rng(320 + num_batches)
    P = rng.random((20000, 3), dtype=np.float32)
    batch = rng.integers(0, num_batches, 20000).astype(np.int32)
    Q = rng.random((256, 3), dtype=np.float32)
    batch_q = rng.integers(0, num_batches, 256).astype(np.int32)
    batch_q[5], batch_q[77], batch_q[200] = -1, num_batches, 2 ** 31 - 1
    Q[9, 1] = np.nan
    return P, batch, Q, batch_q


def twins_case():
    """(P, batch, Q, batch_q): 600 points, the same coordinates present in batch 0 and in batch 1 (rows interleaved), and a
    third batch of 100 others; the queries are 40 of the shared coordinates under each of the three labels."""
    rng = np.random.default_rng(330)
    A = rng.random((250, 3), dtype=np.float32)
    P = np.concatenate([A, A, rng.random((100, 3), dtype=np.float32)])
    batch = np.concatenate([np.zeros(250), np.ones(250), np.full(100, 2)]).astype(np.int32)
    perm = rng.permutation(len(P))
    P, batch = np.ascontiguousarray(P[perm]), np.ascontiguousarray(batch[perm])
    Q = np.ascontiguousarray(np.concatenate([A[:40], A[:40], A[:40]]))
    batch_q = np.repeat(np.arange(3), 40).astype(np.int32)
    return P, batch, Q, batch_q


def nan_case():
    """(P, batch, Q, batch_q, radii): 700 points in 4 batches of which 23 have a NaN; 64 queries of which 5 have one and 4 a
    label no batch has; per-row radii with NaN, inf, 0 and negative entries."""
    rng = np.random.default_rng(340)
    P = rng.random((700, 3), dtype=np.float32)
    batch = rng.integers(0, 4, 700).astype(np.int32)
    for t, row in enumerate(rng.choice(len(P), 23, replace=False)):
        P[row, : 1 + t % 3] = np.nan
    Q = rng.random((64, 3), dtype=np.float32)
    batch_q = rng.integers(0, 4, 64).astype(np.int32)
    for t, row in enumerate((3, 17, 18, 40, 63)):
        Q[row, t % 3] = np.nan
    batch_q[[1, 20, 41, 62]] = (-1, 4, 1000, -(2 ** 31))
    radii = (rng.random(64, dtype=np.float32) * np.float32(0.4)).astype(np.float32)
    radii[[0, 7, 8, 9, 33]] = (np.nan, np.inf, 0, -1, np.finfo(np.float32).max)
    return P, batch, Q, batch_q, radii


# ---- the batched build ---------------------------------------------------------------------------------------------------------------
def build_points(points, batch, num_batches, ids=None, curve=0):
    """Everything TrueKNN.export_tree_ex returns for build(points, ids, batch, num_batches) under that curve, and ``starts``
    (num_batches + 1): tests/lbvh_spec.py's build_points with the batched keys in the place of the plain ones -- one scene box,
    the stable order of the keys, the radix tree, node table and wide pyramid of those keys."""
    import curve_key_host
    import lbvh_spec as ls

    p = ls.pad3(points)
    n = len(p)
    scene, ext = ls.scene_box(p, p)
    key21 = curve_key_host.point_keys(curve_key_host.load(), curve, ls.KEY_LEVELS, p, scene[:3], ext)
    keys = batched_keys(key21, batch, num_batches)
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    bad = np.isnan(p).any(axis=1)
    tree = ls.radix_tree(keys)
    sp = p[order]
    lo, hi = sp.copy(), sp.copy()
    lo[bad[order]], hi[bad[order]] = np.inf, -np.inf
    total = (n + ls.BLOCK - 1) // ls.BLOCK * ls.BLOCK + ls.BLOCK
    records = np.empty((total, 4), np.uint32)
    records[:, :3], records[:, 3] = ls.NAN_BITS, np.int32(-1).view(np.uint32)
    records[:n, :3] = sp.view(np.uint32)
    records[:n][bad[order], :3] = ls.NAN_BITS
    records[:n, 3] = (order if ids is None else np.asarray(ids)[order]).astype(np.int32).view(np.uint32)
    row_slot = np.empty(n, np.int32)
    row_slot[order] = np.arange(n, dtype=np.int32)
    levels, count, wide = ls.wide_pyramid(lo, hi)
    bb = np.uint64(key_bits(num_batches))
    starts = np.searchsorted(keys, np.arange(num_batches + 1, dtype=np.uint64) << (np.uint64(63) - bb), side="left").astype(np.int32)
    return {"n": n, "curve": int(curve), "keys": keys, "prim_id": order.astype(np.int32), "row_slot": row_slot, "points": records,
            "scene": scene, "nan_count": int(bad.sum()), "nodes": ls.node_table(tree, lo, hi), "rope_node": tree["rope_node"],
            "rope_leaf": tree["rope_leaf"], "split_owner": tree["split_owner"], "wide_levels": levels, "wide_count": count,
            "wide_boxes": wide, "starts": starts}
