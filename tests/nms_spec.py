"""What TrueKNN.radius_nms (tknnRadiusNms, include/owlknn_nms.h) must give, restated in numpy, and the cases its tests share.  No
tests here.

Brute force, no tree (``brute``).  In every cloud -- the points of one label; a point's name is its id where ids are given, its row
otherwise --
  * eligible are the points without a NaN coordinate and, where scores are given, without a NaN score;
  * p is within r of q iff sqrt((dx*dx + dy*dy) + dz*dz) <= r, every operation rounded to float32 (query_spec.distance32, the way
    radius_spec.radius_rows computes its rows);
  * the key of a point is (strength, name): the larger strength wins, among equal strengths the smaller name.  The strength is the
    order-preserving image of the score's bits (~u if the sign bit is set, u | 0x80000000 otherwise: -0 < +0), without scores
    murmur3's fmix32 of the name's 32 bits, with ``by_name`` 0 for everybody;
  * the eligible points are walked from the best key down; a point is kept iff no point kept before it is within r of it;
  * cover: a kept point's own name; for an eligible point that is not kept the kept point of its cloud within r with the smallest
    (distance bits, name); -1 for a point that is not eligible.  counts[b]: the kept points of cloud b.
``depth``: 1 for an eligible point that no point of its cloud with a better key has within r, otherwise 1 + the largest depth among
those points; 0 for a point that is not eligible.  The rounds of a call never exceed the largest depth.
"""
import numpy as np

from owlraytracing_amd.datasets import pad_to_3d

import batch_spec
import fps_spec
from query_spec import distance32


def fmix32(h):
    """murmur3's finaliser on uint32 values."""
    h = np.asarray(h).astype(np.uint32).copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def score_image(scores):
    """The uint32 that orders like the float32 scores' bits: -0 below +0, every NaN aside."""
    u = np.asarray(scores, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def keys(names, scores=None, by_name=False):
    """uint64 keys of which the LARGER wins: the strength above the complement of the name's place in the signed order."""
    names = np.asarray(names, np.int64)
    assert not (by_name and scores is not None)
    if scores is not None:
        strength = score_image(scores)
    elif by_name:
        strength = np.zeros(len(names), np.uint32)
    else:
        strength = fmix32(names.astype(np.int32).view(np.uint32))
    order = (names.astype(np.int32).view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
    return (strength.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - order)


def _setup(P, scores, batch, num_batches, ids):
    P = pad_to_3d(np.asarray(P, np.float32))
    n = len(P)
    batch = np.zeros(n, np.int64) if batch is None else np.asarray(batch, np.int64)
    B = (int(batch.max()) + 1 if n else 1) if num_batches is None else int(num_batches)
    names = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    ok = ~np.isnan(P).any(axis=1)
    if scores is not None:
        ok &= ~np.isnan(np.asarray(scores, np.float32))
    return P, n, batch, B, names, ok


def _near(A, q, r):
    """Which rows of A are within r of the point q."""
    with np.errstate(invalid="ignore", over="ignore"):
        return distance32(A, q[None, :]) <= np.float32(r)


def brute(P, r, scores=None, batch=None, num_batches=None, ids=None, by_name=False):
    """dict(keep (n,) bool, cover (n,) int32, counts (B,) int32, eligible, bad_scores) by the sequential greedy loop."""
    P, n, batch, B, names, ok = _setup(P, scores, batch, num_batches, ids)
    key = keys(names, scores, by_name)
    keep = np.zeros(n, bool)
    cover = np.full(n, -1, np.int32)
    counts = np.zeros(B, np.int32)
    for b in range(B):
        rows = np.flatnonzero(ok & (batch == b))
        rows = rows[np.argsort(key[rows], kind="stable")[::-1]]  # from the best key down
        kept = np.zeros(len(rows), np.int64)
        m = 0
        for i in rows:
            if not _near(P[kept[:m]], P[i], r).any():
                kept[m] = i
                m += 1
        kept = kept[:m]
        keep[kept] = True
        counts[b] = m
        cover[kept] = names[kept]
        for i in rows[~keep[rows]]:
            with np.errstate(invalid="ignore", over="ignore"):
                d = distance32(P[kept], P[i][None, :])
            c = np.flatnonzero(d <= np.float32(r))
            cover[i] = names[kept[c[np.lexsort((names[kept[c]], d[c].view(np.uint32)))[0]]]]
    bad = 0 if scores is None else int(np.isnan(np.asarray(scores, np.float32)).sum())
    return {"keep": keep, "cover": cover, "counts": counts, "eligible": int(ok.sum()), "bad_scores": bad}


def depth(P, r, scores=None, batch=None, num_batches=None, ids=None, by_name=False):
    """(n,) int64: the length of the longest chain of points, each within r of and with a better key than the next, that ends in
    the point (0: not eligible)."""
    P, n, batch, B, names, ok = _setup(P, scores, batch, num_batches, ids)
    key = keys(names, scores, by_name)
    out = np.zeros(n, np.int64)
    for b in range(B):
        rows = np.flatnonzero(ok & (batch == b))
        rows = rows[np.argsort(key[rows], kind="stable")[::-1]]
        Q = P[rows]
        dep = np.zeros(len(rows), np.int64)
        for t in range(len(rows)):
            near = _near(Q[:t], Q[t], r)
            dep[t] = 1 + (dep[:t][near].max() if near.any() else 0)
        out[rows] = dep
    return out


_cache = {}


def rows_of(key, make):
    """The spec's rows of a named case, computed once and shared (do not write to them)."""
    if key not in _cache:
        rows = make()
        for a in rows.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = rows
    return _cache[key]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
LATTICE_STEP = np.float32(1.0 / 32)
LINE_STEP = np.float32(1.0 / 64)
LINE_POINTS = 400


def _uniform(n):
    def make():
        return {"P": fps_spec.uniform_case(n, 800 + n), "r": min(0.5, 1.2 * n ** (-1.0 / 3))}  # about seven points within r
    return make


def _random_scores(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def _straddle(scored):
    def make():
        P, batch = fps_spec.straddle_case()
        return {"P": P, "batch": batch, "num_batches": len(fps_spec.STRADDLE_SIZES), "r": 0.15, "scores": _random_scores(len(P), 811) if scored else None}
    return make


def _clouds():
    P, batch, _, _ = batch_spec.clouds_case()  # seven clouds in one unit cube, the first one empty
    return {"P": P, "batch": batch, "num_batches": len(batch_spec.CLOUD_SIZES), "r": 0.12}


def _copies():
    return {"P": np.tile(np.array([[0.3, 0.4, 0.5]], np.float32), (600, 1)), "batch": (np.arange(600) % 2).astype(np.int32), "num_batches": 2, "r": 0.01}


def _lattice(r):
    def make():
        g = np.arange(12, dtype=np.float32) * LATTICE_STEP
        P = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        return {"P": np.ascontiguousarray(P[np.random.default_rng(812).permutation(len(P))]), "r": r}
    return make


def _line(by_name):
    def make():
        P = np.zeros((LINE_POINTS, 3), np.float32)
        P[:, 0] = np.arange(LINE_POINTS, dtype=np.float32) * LINE_STEP
        r = np.float32(1.5) * LINE_STEP
        if by_name:  # names are rows: row i is dominated by row i - 1
            return {"P": P, "r": r, "by_name": True}
        perm = np.random.default_rng(813).permutation(LINE_POINTS)  # the scores rise along the line, the rows are shuffled
        return {"P": np.ascontiguousarray(P[perm]), "r": r, "scores": perm.astype(np.float32)}
    return make


def _ids(below_n):
    def make():
        P, ids = fps_spec.ids_case()
        if below_n:
            ids = np.random.default_rng(814).permutation(len(P)).astype(np.int32)
        return {"P": P, "ids": ids, "r": 0.1, "scores": np.round(_random_scores(len(P), 815) * 4).astype(np.float32) / 4}
    return make


def _nan():
    """800 points in 3 clouds, 21 with a NaN coordinate; scores from a handful of values, -0 and +0 among them, 40 of them NaN."""
    P, batch = fps_spec.nan_case()
    rng = np.random.default_rng(816)
    scores = rng.choice(np.array([-0.0, 0.0, 1.0, -2.5, np.inf, -np.inf, 1e-40, -1e-40], np.float32), len(P)).astype(np.float32)
    scores[rng.choice(len(P), 40, replace=False)] = np.nan
    return {"P": P, "batch": batch, "num_batches": 3, "r": 0.12, "scores": scores}


def _signed_zeros():
    """Eight points in a row within r of each other, scores +0 and -0 alternating: the +0 with the smallest name wins."""
    P = np.zeros((8, 3), np.float32)
    P[:, 1] = np.arange(8, dtype=np.float32) * np.float32(0.001)
    return {"P": P, "r": 0.5, "scores": np.array([-0.0, 0.0] * 4, np.float32)}


def _large_r():
    rng = np.random.default_rng(817)
    return {"P": rng.random((500, 3), dtype=np.float32), "batch": rng.integers(0, 2, 500).astype(np.int32), "num_batches": 2, "r": 4.0}


def _tiny_r():
    return {"P": fps_spec.uniform_case(1000, 818), "r": 1e-6}


def _uniform8000(scored):
    def make():
        return {"P": fps_spec.uniform_case(8000, 819), "r": 0.0668, "scores": _random_scores(8000, 820) if scored else None}  # about ten points within r
    return make


def _planar():
    return {"P": fps_spec.planar_case(), "r": 0.06}


CASES = {
    "uniform1": _uniform(1), "uniform16": _uniform(16), "uniform17": _uniform(17), "uniform1024": _uniform(1024), "uniform1025": _uniform(1025),
    "straddle": _straddle(False), "straddle_scored": _straddle(True), "clouds": _clouds, "copies": _copies,
    "lattice_at_step": _lattice(LATTICE_STEP), "lattice_below_step": _lattice(np.nextafter(LATTICE_STEP, np.float32(0))),
    "line_scored": _line(False), "line_by_name": _line(True), "ids_below_n": _ids(True), "ids_above_n": _ids(False),
    "nan": _nan, "signed_zeros": _signed_zeros, "large_r": _large_r, "tiny_r": _tiny_r,
    "uniform8000": _uniform8000(False), "uniform8000_scored": _uniform8000(True), "planar": _planar,
}


def case(name):
    """dict(P, r, scores, batch, num_batches, ids, by_name) of a named case, the absent entries None / False (shared: do not write)."""
    def make():
        c = {"scores": None, "batch": None, "num_batches": None, "ids": None, "by_name": False}
        c.update(CASES[name]())
        c["r"] = np.float32(c["r"])
        return c
    return rows_of(("case", name), make)


def spec_args(c):
    return dict(scores=c["scores"], batch=c["batch"], num_batches=c["num_batches"], ids=c["ids"], by_name=c["by_name"])


def want(name):
    """brute's result for a named case, computed once."""
    c = case(name)
    return rows_of(("want", name), lambda: brute(c["P"], c["r"], **spec_args(c)))


def max_depth(name):
    c = case(name)
    return int(rows_of(("depth", name), lambda: {"d": depth(c["P"], c["r"], **spec_args(c))})["d"].max(initial=0))
