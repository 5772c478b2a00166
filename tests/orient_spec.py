"""What TrueKNN.orient_normals (tknnOrientNormals, include/owlknn_orient.h) must return, restated in numpy, and the cases its tests
share.  No tests here.

P is the built set, N its normals by row, read as given.  A point is eligible if it has no NaN coordinate and its normal is finite.
  * the graph G on the eligible points: {i, j} is an edge if j is in i's own-points kNN row at k (tests/knn_spec.py self_rows) or i in
    j's, and, with `emst`, if it is a record of the Euclidean forest (tests/emst_spec.py mst); both ends eligible, or it is no edge;
  * c = (nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j in float32 (bitwise symmetric: asserted), w = fmaxf(1 - |c|, 0) with a NaN giving 0 and
    -0 written as +0, s = (c < 0);
  * edges are ordered by the strict key (bits of w, min name, max name); Kruskal over it gives the unique minimum spanning forest T;
  * the root of a component is its point with the largest t = (px*dx + py*dy) + pz*dz (float32, a NaN counts as -inf, -0 equals +0),
    the smallest row among equals; it is flipped iff (nx*dx + ny*dy) + nz*dz < 0;
  * flip[v] = flip[root] ^ the parity of the edges with s = 1 on the tree path root .. v -- computed twice here, by that parity along
    a breadth-first order (flips_by_parity) and by the literal depth-first rule on the normals themselves (flips_by_dfs): the child
    is flipped iff its dot with the ORIENTED parent is < 0; where that dot is zero or a NaN there is no sign to go on and the child
    takes its parent's flip, which is what s = (c < 0) says (negation is exact: the dot with a flipped parent is -c, bit for bit);
  * out[v] = N[v] with the three sign bits toggled iff flip[v]; a point that is not eligible keeps its normal, flip 0, component -1.
n <= 4096.
"""
import numpy as np

import emst_spec as em
import knn_spec as kn
from owlraytracing_amd.datasets import pad_to_3d

MAX_N = 4096
SIGN = np.uint32(0x80000000)


def eligible(P, N):
    P, N = pad_to_3d(np.asarray(P, np.float32)), np.asarray(N, np.float32)
    return ~np.isnan(P).any(axis=1) & np.isfinite(N).all(axis=1)


def dot3(A, B):
    """(ax*bx + ay*by) + az*bz per row, every operation rounded to float32."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = (A[..., 0] * B[..., 0] + A[..., 1] * B[..., 1]) + A[..., 2] * B[..., 2]
    assert c.dtype == np.float32
    return c


def weight_bits(c):
    """(bits of w, s) of the dots c."""
    c = np.asarray(c, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.float32(1) - np.abs(c)
        w = np.where(w > 0, w, np.float32(0)).astype(np.float32)  # fmaxf(w, 0): a NaN gives 0, and a -0 a +0
        s = c < 0
    return w.view(np.uint32), s


_graphs = {}


def graph(key, P, k, ids):
    """(knn edges (m,2), emst edges (m',2)) of a point set as ROWS, computed once per `key`; names[row] is ids[row] or the row."""
    gk = (key, k)
    if gk not in _graphs:
        P = pad_to_3d(np.asarray(P, np.float32))
        n = len(P)
        assert n <= MAX_N
        names = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
        row_of = {int(name): r for r, name in enumerate(names)}
        idx = kn.self_rows(P, k, ids=ids)["idx"]
        i, t = np.nonzero(idx >= 0)
        knn_edges = np.stack([i, np.array([row_of[int(x)] for x in idx[i, t]], np.int64)], axis=1).reshape(-1, 2)
        if ("mst", key) not in _graphs:
            f = em.mst(P, None, ids)
            _graphs[("mst", key)] = np.stack([[row_of[int(x)] for x in f["u"]], [row_of[int(x)] for x in f["v"]]], axis=1).reshape(-1, 2).astype(np.int64)
        _graphs[gk] = (knn_edges, _graphs[("mst", key)])
    return _graphs[gk]


def flips_by_parity(n, root, adj, root_flip, flip):
    """Breadth-first from `root`: flip[child] = flip[parent] ^ s(edge)."""
    flip[root] = root_flip
    seen, queue = {root}, [root]
    for v in queue:
        for to, s in adj[v]:
            if to not in seen:
                seen.add(to)
                flip[to] = flip[v] ^ s
                queue.append(to)
    return seen


def flips_by_dfs(N, root, adj, root_flip, flip):
    """Depth-first on the normals themselves: the child against its ORIENTED parent."""
    oriented = {root: -N[root] if root_flip else N[root]}
    flip[root] = root_flip
    stack = [root]
    while stack:
        v = stack.pop()
        for to, _ in adj[v]:
            if to in oriented:
                continue
            d = dot3(oriented[v], N[to])
            f = True if d < 0 else False if d > 0 else bool(flip[v])  # (zero or NaN: no sign to go on, the child goes with its parent)
            flip[to] = f
            oriented[to] = -N[to] if f else N[to]
            stack.append(to)


def orient(P, N, k, ids=None, direction=(0, 0, 1), emst=True, key=None):
    """dict(normals, flip, component, u, v, w, tree_edges, components, excluded, flipped, candidates, roots)."""
    P, N = pad_to_3d(np.asarray(P, np.float32)), np.ascontiguousarray(N, np.float32)
    n = len(P)
    assert N.shape == (n, 3) and n <= MAX_N
    d = np.asarray(direction, np.float32)
    names = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    ok = eligible(P, N)
    knn_edges, mst_edges = graph(key if key is not None else (P.tobytes(), None if ids is None else names.tobytes()), P, k, ids)
    E = np.concatenate([knn_edges, mst_edges]) if emst else knn_edges
    E = E[ok[E[:, 0]] & ok[E[:, 1]]] if len(E) else E.reshape(0, 2)
    c = dot3(N[E[:, 0]], N[E[:, 1]])
    assert np.array_equal(c.view(np.uint32), dot3(N[E[:, 1]], N[E[:, 0]]).view(np.uint32)), "bitwise symmetric"
    wb, s = weight_bits(c)
    lo, hi = np.minimum(names[E[:, 0]], names[E[:, 1]]), np.maximum(names[E[:, 0]], names[E[:, 1]])
    # duplicates of one edge are one edge (one pair has one weight)
    _, first = np.unique(np.stack([lo, hi], axis=1), axis=0, return_index=True) if len(E) else (None, np.zeros(0, np.int64))
    E, wb, s, lo, hi = E[first], wb[first], s[first], lo[first], hi[first]
    parent = list(range(n))
    adj = [[] for _ in range(n)]
    u, v, w = [], [], []
    for e in np.lexsort((hi, lo, wb)):
        a, b = em._find(parent, int(E[e, 0])), em._find(parent, int(E[e, 1]))
        if a != b:
            parent[max(a, b)] = min(a, b)  # (the smaller row stays root)
            u.append(lo[e]), v.append(hi[e]), w.append(wb[e])
            adj[int(E[e, 0])].append((int(E[e, 1]), bool(s[e])))
            adj[int(E[e, 1])].append((int(E[e, 0]), bool(s[e])))
    component = np.full(n, -1, np.int32)
    for r in np.flatnonzero(ok):
        component[r] = em._find(parent, int(r))
    t = dot3(P, d[None, :])
    t = np.where(np.isnan(t), np.float32(-np.inf), t)
    toward = dot3(N, d[None, :])
    flip, flip_dfs, roots = np.zeros(n, bool), np.zeros(n, bool), []
    for comp in np.unique(component[ok]):
        rows = np.flatnonzero(component == comp)
        root = int(rows[t[rows] == t[rows].max()].min())  # (float comparison: -0 equals +0)
        with np.errstate(invalid="ignore"):
            root_flip = bool(toward[root] < 0)
        seen = flips_by_parity(n, root, adj, root_flip, flip)
        assert sorted(seen) == rows.tolist()
        flips_by_dfs(N, root, adj, root_flip, flip_dfs)
        roots.append(root)
    assert np.array_equal(flip, flip_dfs), "parity along the path and the depth-first rule agree"
    out = N.view(np.uint32) ^ np.where(flip, SIGN, np.uint32(0))[:, None]
    return {"normals": out.view(np.float32), "flip": flip.astype(np.uint8), "flip_dfs": flip_dfs.astype(np.uint8), "component": component,
            "u": np.array(u, np.int32), "v": np.array(v, np.int32), "w": np.array(w, np.uint32).view(np.float32), "tree_edges": len(u),
            "components": int(ok.sum()) - len(u), "excluded": int(n - ok.sum()), "flipped": int(flip.sum()),
            "candidates": n * k + (n - 1 if emst else 0), "roots": np.array(roots, np.int64)}


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def random_normals(n, seed):
    """n unit-length (to rounding) normals in random directions."""
    g = np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)
    return np.ascontiguousarray(g / np.linalg.norm(g, axis=1, keepdims=True).astype(np.float32))


def random_signs(N, seed):
    """N with each row negated or not, at random: negation is exact."""
    neg = np.random.default_rng(seed).random(len(N)) < 0.5
    return np.ascontiguousarray(np.where(neg[:, None], -N, N).astype(np.float32))


def sphere_points(n, seed, centre=(0, 0, 0)):
    """(P, the outward unit normals): n points of a unit sphere about `centre`; the normal is the unit vector that was shifted."""
    U = random_normals(n, seed)
    return np.ascontiguousarray(U + np.float32(centre)), U


TINY_N = em.TINY_N


def tiny_case(n, big):
    return {"key": "tiny%d" % n, "P": em.tiny_case(n), "N": random_normals(n, 300 + n), "k": min(n + 2, kn.K_MAX) if big else 1}


def sphere_case(noisy):
    P, U = sphere_points(2000, 310)
    N = U
    if noisy:
        N = U + np.random.default_rng(311).standard_normal(U.shape).astype(np.float32) * np.float32(0.4)
        N = np.ascontiguousarray(N / np.linalg.norm(N, axis=1, keepdims=True).astype(np.float32))
    return {"key": "sphere", "P": P, "N": random_signs(N, 312), "k": 8, "outward": U}


def plane_case(above):
    """All normals identical: every weight is 0, every t is 0 -- the names alone decide the tree, the rows the root."""
    from owlraytracing_amd import datasets

    P = datasets.uniform3d(1000, seed=313)
    P[:, 2] = 0
    N = np.ascontiguousarray(np.tile(np.float32([[0, 0, 1]]), (len(P), 1)))
    return {"key": "plane_above" if above else "plane_below", "P": P, "N": N, "k": 6, "ids": em.permuted_ids(len(P), above)}


def bad_case():
    """knn_spec's 700 points with 23 NaN ones, and normals with NaN, infinite and zero rows."""
    P = em.nan_case()
    N = random_normals(len(P), 314)
    rng = np.random.default_rng(315)
    rows = rng.choice(np.flatnonzero(~np.isnan(P).any(axis=1)), 40, replace=False)  # (40 points that are not left out already)
    for t, r in enumerate(rows[:10]):
        N[r, t % 3] = np.nan
    for t, r in enumerate(rows[10:20]):
        N[r, t % 3] = np.inf if t % 2 else -np.inf
    N[rows[20:30]] = 0
    N[rows[30:40]] = np.float32([-0.0, 0.0, -0.0])
    return {"key": "bad", "P": P, "N": N, "k": 8}


def two_spheres_case(emst):
    A, UA = sphere_points(1000, 316)
    B, UB = sphere_points(1000, 317, centre=(10, 0, 0))
    return {"key": "two_spheres", "P": np.concatenate([A, B]), "N": random_signs(np.concatenate([UA, UB]), 318), "k": 8, "emst": emst,
            "outward": np.concatenate([UA, UB])}


def lattice_case(direction=(0, 0, 1)):
    P = em.lattice_case()
    return {"key": "lattice", "P": P, "N": random_normals(len(P), 319), "k": 6, "direction": direction}


def duplicates_case():
    P = em.duplicates_case()
    return {"key": "duplicates", "P": P, "N": random_normals(len(P), 320), "k": 16}


def uniform4096_case():
    P = em.point_set("uniform4096")
    return {"key": "uniform4096", "P": P, "N": random_normals(len(P), 321), "k": 16}


CASES = {}
for _n in TINY_N:
    CASES["tiny%d_k1" % _n] = lambda n=_n: tiny_case(n, False)
    CASES["tiny%d_kbig" % _n] = lambda n=_n: tiny_case(n, True)
CASES.update({
    "sphere": lambda: sphere_case(False),
    "sphere_noisy": lambda: sphere_case(True),
    "plane_ids_below_n": lambda: plane_case(False),
    "plane_ids_above_n": lambda: plane_case(True),
    "lattice": lattice_case,
    "duplicates": duplicates_case,
    "bad_inputs": bad_case,
    "two_spheres_no_emst": lambda: two_spheres_case(False),
    "two_spheres": lambda: two_spheres_case(True),
    "direction_zero": lambda: dict(sphere_case(True), direction=(0, 0, 0)),
    "direction_tie": lambda: lattice_case(direction=(1, 0, 0)),  # 144 lattice points share the largest x
    "uniform4096": uniform4096_case,
})
SIGN_FREE = ("sphere_noisy", "duplicates", "tiny17_kbig")  # random normals: no dot is exactly zero, the output is free of the input's signs
SMALL = tuple(name for name in CASES if name.startswith("tiny")) + ("bad_inputs", "plane_ids_above_n")  # quick on the host

_cache = {}


def case(name):
    """(the case: P, N, k, ids, direction, emst [, outward]; the spec's answer), computed once and shared (do not write to them)."""
    if name not in _cache:
        c = dict({"ids": None, "direction": (0, 0, 1), "emst": True}, **CASES[name]())
        want = orient(c["P"], c["N"], c["k"], ids=c["ids"], direction=c["direction"], emst=c["emst"], key=c["key"])
        for a in list(want.values()) + [c["P"], c["N"]]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (c, want)
    return _cache[name]
