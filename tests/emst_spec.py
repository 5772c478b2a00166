"""What TrueKNN.emst (tknnEmst, include/owlknn_emst.h) must return, restated in numpy, and the cases its tests share.  No tests here.

P is the built set, E its eligible points: a point is eligible if it has no NaN coordinate and, with core distances, its core
distance is finite and >= 0 (-0 counts as 0).
  * the weight of {i, j} is d(i, j) = sqrt((dx*dx + dy*dy) + dz*dz), every operation rounded to float32 (bitwise symmetric); with
    core distances w = max(max(d, core[i]), core[j]).  A distance that is not finite is no edge (an overflowing one included);
  * edges are ordered by the strict key (bits of w as uint32, min(name_i, name_j), max(name_i, name_j)), name = id where ids are
    given, row otherwise;
  * under a strict order the minimum spanning forest is unique: Kruskal over the key with a host union-find gives it.  The records
    are (u, v, w) with u < v (names), ascending by the key; component[row] = the smallest row of the point's component, -1 for a
    point that is not eligible.
"""
import numpy as np

from owlraytracing_amd.datasets import pad_to_3d

MAX_N = 4096


def eligible(P, core=None):
    P = pad_to_3d(np.asarray(P, np.float32))
    ok = ~np.isnan(P).any(axis=1)
    if core is not None:
        core = np.asarray(core, np.float32)
        with np.errstate(invalid="ignore"):
            ok &= np.isfinite(core) & (core >= 0)
    return ok


def weights(P, core=None):
    """(W (n,n) float32, eligible (n,) bool): W[i, j] the weight of {i, j}, +inf where there is no edge."""
    P = pad_to_3d(np.asarray(P, np.float32))
    n = len(P)
    assert n <= MAX_N
    ok = eligible(P, core)
    with np.errstate(invalid="ignore", over="ignore"):
        d = P[None, :, :] - P[:, None, :]  # float32 - float32
        x, y, z = d[..., 0], d[..., 1], d[..., 2]
        W = np.sqrt(((x * x) + (y * y)) + (z * z), dtype=np.float32)
    assert W.dtype == np.float32
    edge = np.isfinite(W) & ok[:, None] & ok[None, :]
    np.fill_diagonal(edge, False)
    if core is not None:
        c = np.where(ok, np.asarray(core, np.float32), np.float32(0)) + np.float32(0)  # (-0 + 0 = +0)
        W = np.maximum(np.maximum(W, c[:, None]), c[None, :])
    W = np.where(edge, W, np.float32(np.inf)).astype(np.float32)
    assert np.array_equal(W.view(np.uint32), W.T.view(np.uint32)), "bitwise symmetric"
    return W, ok


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def mst(P, core=None, ids=None):
    """dict(u, v (edges,) int32, w (edges,) float32, edges, components, excluded, component (n,) int32): Kruskal over the strict
    key.  The edges are taken in slices of ascending weight (the first slices hold the whole tree on ordinary sets), each
    sorted by the full key."""
    P = pad_to_3d(np.asarray(P, np.float32))
    n = len(P)
    W, ok = weights(P, core)
    names = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    assert len(np.unique(names)) == n and (names >= 0).all()
    i, j = np.triu_indices(n, 1)
    wb = W[i, j].view(np.uint32)
    keep = wb < np.float32(np.inf).view(np.uint32)
    i, j, wb = i[keep], j[keep], wb[keep]
    lo, hi = np.minimum(names[i], names[j]), np.maximum(names[i], names[j])
    parent = list(range(n))
    want = int(ok.sum()) - 1
    u, v, w = [], [], []
    done = np.zeros(len(wb), bool)
    take = 8 * n
    while len(u) < want and not done.all():
        left = np.flatnonzero(~done)
        if len(left) > take:
            cut = np.partition(wb[left], take - 1)[take - 1]
            left = left[wb[left] <= cut]  # (every edge at the cut weight: the slice is closed under the key's ties)
        done[left] = True
        lab = np.array([_find(parent, r) for r in range(n)])
        left = left[lab[i[left]] != lab[j[left]]]  # (an edge inside a component is never taken: less to sort)
        for e in left[np.lexsort((hi[left], lo[left], wb[left]))]:
            a, b = _find(parent, int(i[e])), _find(parent, int(j[e]))
            if a != b:
                parent[max(a, b)] = min(a, b)
                u.append(lo[e]), v.append(hi[e]), w.append(wb[e])
        take *= 4
    component = np.full(n, -1, np.int32)
    for r in np.flatnonzero(ok):
        component[r] = _find(parent, int(r))  # (the smaller row stays root)
    return {"u": np.array(u, np.int32), "v": np.array(v, np.int32), "w": np.array(w, np.uint32).view(np.float32), "edges": len(u),
            "components": int(ok.sum()) - len(u), "excluded": int(n - ok.sum()), "component": component}


def labels_of_edges(n, u, v):
    """component[row] = the smallest row joined to it by the edges (u, v) over rows."""
    parent = list(range(n))
    for a, b in zip(u.tolist(), v.tolist()):
        a, b = _find(parent, a), _find(parent, b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([_find(parent, r) for r in range(n)], np.int32)


def round_bound(n):
    """ceil(log2 n) + 1: the rounds Boruvka needs at most under a strict order."""
    return int(np.ceil(np.log2(n))) + 1 if n > 1 else 1


def core_distances(P, min_samples, ids=None):
    """The distance to the (min_samples - 1)-th nearest other point (tests/knn_spec.py's own rows): sklearn's core distance."""
    import knn_spec as kn

    return np.ascontiguousarray(kn.self_rows(P, min_samples - 1, ids=ids)["dist"][:, -1])


_cache = {}


def case(name):
    """(P, core, ids, the spec's forest) of a named case (CASES), computed once and shared (do not write to them)."""
    if name not in _cache:
        P, core, ids = CASES[name]()
        want = mst(P, core, ids)
        for a in want.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (P, core, ids, want)
    return _cache[name]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
SET_NAMES = ("uniform", "mixture", "planar", "collinear")


def point_set(name):
    from owlraytracing_amd import datasets

    if name == "uniform":
        return datasets.uniform3d(2048, seed=81)
    if name == "mixture":  # three well separated clusters: late rounds have few, large components
        return datasets.gaussian_mixture3d(3000, components=3, sigma=0.02, seed=82)
    if name == "planar":
        P = datasets.uniform3d(2048, seed=83)
        P[:, 2] = 0
        return P
    if name == "collinear":
        t = np.random.default_rng(84).random(500, dtype=np.float32)
        return np.ascontiguousarray(np.stack([t, t * np.float32(0.5), t * np.float32(0.25)], axis=1))
    if name == "uniform4096":
        return datasets.uniform3d(4096, seed=85)
    raise KeyError(name)


def lattice_case():
    """12^3 points at spacing 1/32 (exact in fp32), rows shuffled: every nearest distance is tied."""
    g = np.arange(12, dtype=np.float32) / np.float32(32)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(P[np.random.default_rng(86).permutation(len(P))])


def duplicates_case():
    """1 000 uniform points of which 70, spread over the rows, are one point: zero weights, decided by names."""
    import knn_spec as kn

    return kn.duplicates_case()[0]


def identical_case():
    return np.ascontiguousarray(np.tile(np.float32([[0.25, 0.5, 0.75]]), (100, 1)))


TINY_N = (1, 2, 3, 16, 17, 63, 64, 65)


def tiny_case(n):
    return np.random.default_rng(87 + n).random((n, 3), dtype=np.float32)


def nan_case():
    """700 uniform points of which 23 have a NaN in one, two or three coordinates."""
    import knn_spec as kn

    return kn.nan_case()[0]


def far_case():
    """Two clusters of 300 points at x = +-3e38: every distance between them overflows, the forest has two trees."""
    rng = np.random.default_rng(88)
    P = rng.random((600, 3), dtype=np.float32)
    P[:, 0] = np.where(rng.random(600) < 0.5, np.float32(3e38), np.float32(-3e38))
    return np.ascontiguousarray(P)


def permuted_ids(n, above):
    """A permutation of 0 .. n-1 as ids, or (above) ids >= n in no order of the rows."""
    p = np.random.default_rng(89).permutation(n)
    return (p * 3 + 1_000_000 if above else p).astype(np.int32)


def bad_core(core):
    """`core` with a NaN, a negative, an infinite and a -0 entry: the first three exclude their points."""
    core = np.array(core, np.float32)
    core[5], core[77], core[130], core[200] = np.nan, -1.0, np.inf, -0.0
    return core


MIN_SAMPLES = 6  # the mutual cases: core = the 5th column of the points' own kNN rows


def _mutual(P, bad=False):
    core = core_distances(P, MIN_SAMPLES)
    return P, bad_core(core) if bad else core, None


CASES = {name: (lambda name=name: (point_set(name), None, None)) for name in SET_NAMES + ("uniform4096",)}
CASES.update({"tiny%d" % n: (lambda n=n: (tiny_case(n), None, None)) for n in TINY_N})
CASES.update({
    "lattice": lambda: (lattice_case(), None, None),
    "duplicates": lambda: (duplicates_case(), None, None),
    "identical": lambda: (identical_case(), None, None),
    "nan": lambda: (nan_case(), None, None),
    "far": lambda: (far_case(), None, None),
    "ids_below_n": lambda: (duplicates_case(), None, permuted_ids(1000, False)),
    "ids_above_n": lambda: (duplicates_case(), None, permuted_ids(1000, True)),
    "mutual_uniform": lambda: _mutual(point_set("uniform")),
    "mutual_duplicates": lambda: _mutual(duplicates_case()),
    "mutual_bad_cores": lambda: _mutual(point_set("uniform"), bad=True),
})
NO_ZERO_WEIGHTS = SET_NAMES + ("lattice", "far", "nan", "mutual_uniform", "mutual_bad_cores")  # scipy drops zero entries
