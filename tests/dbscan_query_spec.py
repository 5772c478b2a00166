"""What TrueKNN.dbscan_query (tknnDbscanQuery) must return, restated in numpy, and the point sets its tests run on.  No tests here.

Given the built set P, core_label[row] (>= 0: core with that label, < 0: not core), eps and queries Q, with dist the fp32
formula sqrt((dx*dx + dy*dy) + dz*dz) (query_spec.distance32):
  * labels[j] = the smallest core_label[p] over the core points p with dist(p, q_j) <= eps, -1 if there is none;
  * counts[j] = the number of points p of P, core or not, with dist(p, q_j) <= eps;
  * nothing is "self": a point of P that coincides with q_j is a neighbour at distance 0;
  * a NaN coordinate on either side makes the distance NaN, which is not <= eps: a NaN query gets -1 and 0, NaN points of P
    are nobody's neighbour.
Brute force: every pair's distance is computed.  The clusterings come from oracle.dbscan (tests/test_dbscan_query_expectations.py
holds the two against each other with Q = P).
"""
import numpy as np

import oracle
from owlraytracing_amd import datasets
from owlraytracing_amd.datasets import pad_to_3d

from query_spec import distance32


def query_labels(P, core_label, eps, Q, block=256):
    """(labels (m,) int32, counts (m,) int32) of the queries Q against P with the caller-decided core labels."""
    P, Q = pad_to_3d(np.asarray(P, np.float32)), pad_to_3d(np.asarray(Q, np.float32))
    core_label = np.asarray(core_label, np.int32)
    assert core_label.shape == (len(P),)
    eps = np.float32(eps)
    m = len(Q)
    labels, counts = np.full(m, -1, np.int32), np.zeros(m, np.int32)
    none = np.int64(2) ** 31  # (above every int32: 2**31 - 1 is a label like any other)
    core = core_label >= 0
    core_label = core_label.astype(np.int64)
    for s in range(0, m, block):
        with np.errstate(invalid="ignore", over="ignore"):
            near = distance32(P[None, :, :], Q[s:s + block, None, :]) <= eps  # (NaN <= eps is False)
        counts[s:s + block] = near.sum(axis=1)
        best = np.where(near & core[None, :], core_label[None, :], none).min(axis=1) if len(P) else np.full(near.shape[0], none)
        labels[s:s + block] = np.where(best == none, -1, best)
    return labels, counts


def nearest_core_label(P, core_label, eps, Q):
    """(m,) int32: the label of the NEAREST core point within eps (smallest row among equally near ones), -1 if none --
    what a kernel that does not look for the smallest label would return."""
    P, Q = pad_to_3d(np.asarray(P, np.float32)), pad_to_3d(np.asarray(Q, np.float32))
    core_label = np.asarray(core_label, np.int32)
    rows = np.flatnonzero(core_label >= 0)
    out = np.full(len(Q), -1, np.int32)
    if not len(rows):
        return out
    for j in range(len(Q)):
        with np.errstate(invalid="ignore", over="ignore"):
            d = distance32(P[rows], Q[j])
        d = np.where(np.isnan(d), np.float32(np.inf), d)
        t = int(np.argmin(d))
        if d[t] <= np.float32(eps):
            out[j] = core_label[rows[t]]
    return out


def clusters_reached(P, core_label, eps, Q):
    """(m,) int: how many different labels the core points within eps of each query carry."""
    P, Q = pad_to_3d(np.asarray(P, np.float32)), pad_to_3d(np.asarray(Q, np.float32))
    core_label = np.asarray(core_label, np.int32)
    out = np.zeros(len(Q), np.int64)
    for j in range(len(Q)):
        with np.errstate(invalid="ignore", over="ignore"):
            near = (distance32(P, Q[j]) <= np.float32(eps)) & (core_label >= 0)
        out[j] = len(np.unique(core_label[near]))
    return out


def mixture_draw(n, components, sigma, seed, draw_seed):
    """n points of the mixture datasets.gaussian_mixture3d(.., components, sigma, seed) draws from -- the same means --, drawn
    with another generator."""
    means = np.random.default_rng(seed).random((components, 3))
    rng = np.random.default_rng(draw_seed)
    which = rng.integers(0, components, n)
    return (means[which] + rng.normal(0.0, sigma, (n, 3))).astype(np.float32)


def _case(name, P, Q, eps, min_pts):
    P, Q = np.ascontiguousarray(P, np.float32), np.ascontiguousarray(Q, np.float32)
    eps = float(np.float32(eps))
    ref = oracle.dbscan(P, eps, min_pts)
    core_label = np.where(ref["core"], ref["labels"], -1).astype(np.int32)
    return {"name": name, "P": P, "Q": Q, "eps": eps, "min_pts": int(min_pts), "core_label": core_label, "oracle": ref}


SLAB_EPS, SLAB_MIN_PTS = 0.05, 5
MIXTURE = dict(components=5, sigma=0.03, seed=9)  # tests/test_dbscan.py::test_spec_invariants: eps 0.02, min_pts 4
EDGE_M = (1, 63, 64, 65, 255, 256, 257)  # the wave and workgroup edges of the query kernel


def _slabs():
    rng = np.random.default_rng(41)
    eps = np.float32(SLAB_EPS)
    size = np.float32([0.3, 0.5, 0.5])
    pitch = np.float32(0.3) + np.float32(1.2) * eps
    slabs = []
    for k in range(3):
        s = rng.random((4000, 3), dtype=np.float32) * size
        s[:, 0] += np.float32(k) * pitch
        slabs.append(s)
    P = np.concatenate(slabs)[rng.permutation(12000)]
    planes = np.float32([0.3 + 0.6 * SLAB_EPS, 0.3 + 0.6 * SLAB_EPS + float(pitch)])  # the middles of the two gaps
    gap = rng.random((600, 3), dtype=np.float32) * size
    gap[:, 0] = planes[rng.integers(0, 2, 600)] + (rng.random(600, dtype=np.float32) * np.float32(0.4) - np.float32(0.2)) * eps
    lo, hi = P.min(axis=0) - 2 * eps, P.max(axis=0) + 2 * eps
    wide = (lo + rng.random((600, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    copies = P[rng.choice(len(P), 300, replace=False)]
    return [_case("slabs", P, np.concatenate([gap, wide, copies]), SLAB_EPS, SLAB_MIN_PTS)]


def _mixture():
    P = datasets.gaussian_mixture3d(3000, **MIXTURE)
    other = mixture_draw(1000, MIXTURE["components"], MIXTURE["sigma"], MIXTURE["seed"], 42)
    return [_case("mixture", P, np.concatenate([P, other]), 0.02, 4)]


def _tiny():
    rng = np.random.default_rng(43)
    cases = []
    for n, min_pts in ((1, 1), (2, 1), (2, 2), (5, 2)):
        P = np.float32(0.4) + rng.random((n, 3), dtype=np.float32) * np.float32(0.05)
        Q = np.concatenate([P, P + np.float32(0.01), np.float32(0.4) + rng.random((20, 3), dtype=np.float32) * np.float32(0.2),
                            np.float32([[5, 5, 5], [-3, 0.4, 0.4]])])
        cases.append(_case("n%d_minpts%d" % (n, min_pts), P, Q, 0.06, min_pts))
    P = rng.random((5, 3), dtype=np.float32)
    cases.append(_case("no_core_point", P, np.concatenate([P, rng.random((30, 3), dtype=np.float32)]), 0.5, 6))
    same = np.tile(np.float32([[0.3, 0.4, 0.5]]), (64, 1))
    Q = np.concatenate([same[:3], same[:1] + np.float32([[0.02, 0, 0]]), same[:1] + np.float32([[0.5, 0, 0]]), rng.random((20, 3), dtype=np.float32)])
    cases.append(_case("duplicates64", same, Q, 0.05, 4))
    return cases


def _nan():
    rng = np.random.default_rng(44)
    P = datasets.uniform3d(1000, seed=45)
    bad = rng.choice(1000, 7, replace=False)
    P[bad, rng.integers(0, 3, 7)] = np.nan
    finite = np.flatnonzero(~np.isnan(P).any(axis=1))
    Qn = rng.random((5, 3), dtype=np.float32)
    Qn[np.arange(5), [0, 1, 2, 0, 2]] = np.nan
    Qn[3] = np.nan
    Q = np.concatenate([rng.random((200, 3), dtype=np.float32), Qn, P[rng.choice(finite, 50, replace=False)]])
    return [_case("nan", P, Q[rng.permutation(len(Q))], 0.1, 3)]


def _edges():
    rng = np.random.default_rng(46)
    P = datasets.uniform3d(2048, seed=47)
    cases = []
    for m in EDGE_M:
        Q = rng.random((m, 3), dtype=np.float32)
        out = rng.random(m) < 0.3  # up to ten scene extents outside the box, near it and far from it
        Q[out] = (rng.random((int(out.sum()), 3)) * rng.choice([1.2, 3.0, 21.0], (int(out.sum()), 1)) - rng.choice([0.1, 1.0, 10.0], (int(out.sum()), 1))).astype(np.float32)
        if m >= 63:
            Q[-1] = np.float32([11, 11, 11])
            Q[0] = np.float32([-10, 0.5, 0.5])
        cases.append(_case("m%d" % m, P, Q, 0.08, 4))
    return cases


SET_NAMES = ("slabs", "mixture", "tiny", "nan", "edges")
_MAKERS = {"slabs": _slabs, "mixture": _mixture, "tiny": _tiny, "nan": _nan, "edges": _edges}
_cache = {}


def cases(name):
    """The cases of a named set, each dict(name, P, Q, eps, min_pts, core_label, oracle, labels, counts): labels and counts are
    the spec's, computed once and shared (do not write to them)."""
    if name not in _cache:
        made = _MAKERS[name]()
        for c in made:
            c["labels"], c["counts"] = query_labels(c["P"], c["core_label"], c["eps"], c["Q"])
            for key in ("labels", "counts"):
                c[key].setflags(write=False)
        _cache[name] = made
    return _cache[name]
