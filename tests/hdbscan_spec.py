"""What tknnLinkage, tknnHdbscanLabels and tknnHdbscan (include/owlknn_hdbscan.h) must return, restated in numpy, the contraction
rounds of csrc/linkage.hip restated next to the sequential union-find they must equal, and the cases the tests share.  No tests
here.

The input is a forest over the vertices 0 .. n-1 as `edges` records (u, v, w) in ascending order of tknnEmst's strict key: record i
has rank i.  The nodes of the dendrogram are the leaves 0 .. n-1 and the node n + i of record i.
  * dendrogram: Kruskal in record order.  parent[x] = the node that absorbs x (-1 for a root), left[i] < right[i] the two children
    of node n + i, size[i] the leaves below it.
  * labels: the excess-of-mass selection over the condensed tree, spelled out in labels() below.
"""
import numpy as np

FLT_MIN = float(np.float32(2.0) ** -126)


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def dendrogram(n, u, v):
    """dict(parent (n + edges,), left, right, size (edges,), all int32): a sequential union-find over the records in order."""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    E = len(u)
    parent = np.full(n + E, -1, np.int32)
    left, right, size = np.zeros(E, np.int32), np.zeros(E, np.int32), np.zeros(E, np.int32)
    uf, top, sz = list(range(n)), list(range(n)), [1] * n
    for e in range(E):
        a, b = _find(uf, int(u[e])), _find(uf, int(v[e]))
        assert a != b, "the records are a forest"
        ta, tb = top[a], top[b]
        parent[ta] = parent[tb] = n + e
        left[e], right[e], size[e] = min(ta, tb), max(ta, tb), sz[a] + sz[b]
        r = min(a, b)
        uf[max(a, b)] = r
        top[r], sz[r] = n + e, size[e]
    return {"parent": parent, "left": left, "right": right, "size": size}


def linkage_matrix(d, w):
    """scipy's Z of a spanning tree: (left, right, w, size) as float64 rows."""
    return np.stack([d["left"].astype(np.float64), d["right"].astype(np.float64), np.asarray(w, np.float64), d["size"].astype(np.float64)], axis=1)


NONE = np.iinfo(np.int64).max


def contraction(n, u, v, max_rounds=64):
    """The same dendrogram in contraction rounds, as csrc/linkage.hip builds it: dict(parent, left, right, size, rounds, absorbed
    (per round), host_edges).  Every numbered step is one kernel there; every loop over records or supervertices here is one thread
    per element there.

    State: sv[vertex] its supervertex (a vertex id), top[c] / ssize[c] of a supervertex c the dendrogram node of its latest merge
    (or the leaf) and its leaves, alive[e].  Invariant: a supervertex is a Kruskal cluster -- its inner records all rank below its
    top, every record that leaves it ranks above."""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    E = len(u)
    parent = np.full(n + E, -1, np.int64)
    size = np.zeros(E, np.int64)
    sv, top, ssize = np.arange(n), np.arange(n), np.ones(n, np.int64)
    alive = np.ones(E, bool)
    rounds, absorbed_per_round = 0, []
    while alive.any() and rounds < max_rounds:
        ids = np.flatnonzero(alive)
        a, b = sv[u[ids]], sv[v[ids]]
        # 1. m[c] = the smallest alive rank at supervertex c
        m = np.full(n, NONE)
        np.minimum.at(m, a, ids)
        np.minimum.at(m, b, ids)
        sel = (m[a] == ids) | (m[b] == ids)
        # 2. c points to the other end of m[c]; of a mutual pair the smaller id is the root; the group is the root reached
        g = np.arange(n)
        has = np.flatnonzero(m != NONE)
        ea = m[has]
        other = np.where(sv[u[ea]] == has, sv[v[ea]], sv[u[ea]])
        mutual = m[other] == ea
        g[has] = np.where(mutual & (has < other), has, other)
        while True:  # (pointer jumping: ranks fall strictly along the pointers, so this ends at the roots)
            gg = g[g]
            if np.array_equal(gg, g):
                break
            g = gg
        # 3. T[group] = the smallest rank of a record that is alive, not selected, and has an end in the group
        T = np.full(n, NONE)
        np.minimum.at(T, g[a[~sel]], ids[~sel])
        np.minimum.at(T, g[b[~sel]], ids[~sel])
        # 4. the selected records below their group's T are absorbed, as a chain in (group, rank) order
        take = sel & (ids < T[g[a]])
        ab, ga = ids[take], g[a[take]]
        order = np.lexsort((ab, ga))
        ab, ga = ab[order], ga[order]
        ca, cb = sv[u[ab]], sv[v[ab]]
        chose_a, chose_b = m[ca] == ab, m[cb] == ab
        contrib = np.where(chose_a, ssize[ca], 0) + np.where(chose_b, ssize[cb], 0)
        first = np.r_[True, ga[1:] != ga[:-1]] if len(ab) else np.zeros(0, bool)
        run = np.cumsum(contrib)
        base = np.maximum.accumulate(np.where(first, run - contrib, 0)) if len(ab) else run
        seg = run - base  # the segmented inclusive sum
        size[ab] = seg
        parent[top[ca[chose_a]]] = n + ab[chose_a]
        parent[top[cb[chose_b]]] = n + ab[chose_b]
        later = np.flatnonzero(~first)
        parent[n + ab[later - 1]] = n + ab[later]
        alive[ab] = False
        # 5. the supervertices whose record was absorbed become their group; its top and size are the chain's last record's
        gone = np.zeros(n, bool)
        gone[has] = ~alive[m[has]]
        last = np.r_[first[1:], True] if len(ab) else first
        top[ga[last]], ssize[ga[last]] = n + ab[last], seg[last]
        sv = np.where(gone[sv], g[sv], sv)
        rounds += 1
        absorbed_per_round.append(len(ab))
    host_edges = int(alive.sum())
    uf = {}
    for e in np.flatnonzero(alive):  # what the rounds left: a sequential union-find over the supervertices
        a, b = _find_dict(uf, int(sv[u[e]])), _find_dict(uf, int(sv[v[e]]))
        parent[top[a]] = parent[top[b]] = n + e
        size[e] = ssize[a] + ssize[b]
        r = min(a, b)
        uf[max(a, b)] = r
        top[r], ssize[r] = n + e, size[e]
    left, right = np.full(E, NONE), np.full(E, -1)
    kids = np.flatnonzero(parent >= 0)
    np.minimum.at(left, parent[kids] - n, kids)
    np.maximum.at(right, parent[kids] - n, kids)
    return {"parent": parent.astype(np.int32), "left": left.astype(np.int32), "right": right.astype(np.int32), "size": size.astype(np.int32),
            "rounds": rounds, "absorbed": absorbed_per_round, "host_edges": host_edges}


def _find_dict(uf, x):
    while uf.get(x, x) != x:
        x = uf[x]
    return x


def labels(n, u, v, w, min_cluster_size):
    """HDBSCAN's labels of the forest (eom, no single cluster): dict(labels (n,) int32, lam (n,) float64, clusters, noise,
    condensed_clusters, stability {head node: float}, margin, dendrogram).

    size(x) = leaves below x, big(x) = size >= min_cluster_size; an internal node is a split iff both its children are big;
    lambda(x) = 1 / float64(w(x)), w = 0 replaced by FLT_MIN.  A cluster head is a big root or a big child of a split; its cluster
    is the head and the chain of only-big children below it, down to a split or to a node without a big child; birth(h) =
    lambda(parent(h)), 0 for a root.  A point p leaves the cluster of a(p), its lowest big strict ancestor, at lambda(a(p)); no
    such ancestor: noise.  stability(C) = sum over the points that leave C of (lambda_p - birth) + [a split s ends C] size(s) *
    (lambda(s) - birth).  Children before parents: S(C) = max(stability(C), S(c1) + S(c2)); C wins iff it has no children or its
    stability >= the children's sum; a root cluster never wins.  A point's cluster is the highest winning ancestor-or-self of
    the cluster it left, none: -1; clusters are numbered by their smallest labelled vertex, ascending."""
    d = dendrogram(n, u, v)
    E = len(d["size"])
    N = n + E
    parent = d["parent"].astype(np.int64)
    nsize = np.r_[np.ones(n, np.int64), d["size"].astype(np.int64)]
    big = nsize >= min_cluster_size
    lam_node = np.zeros(N)
    wd = np.asarray(w, np.float32).astype(np.float64)
    lam_node[n:] = 1.0 / np.where(wd == 0, FLT_MIN, wd)
    split = np.zeros(N, bool)
    split[n:] = big[d["left"]] & big[d["right"]]
    head = big & ((parent < 0) | split[np.maximum(parent, 0)])
    a = np.full(n, -1, np.int64)
    for p in range(n):
        x = parent[p]
        while x >= 0 and not big[x]:
            x = parent[x]
        a[p] = x
    lam = np.where(a >= 0, lam_node[np.maximum(a, 0)], 0.0)
    cl = np.full(N, -1, np.int64)
    for x in range(N - 1, -1, -1):  # (a parent has the higher number)
        if big[x]:
            cl[x] = x if head[x] else cl[parent[x]]
    heads = np.flatnonzero(head)
    birth = {int(h): (lam_node[parent[h]] if parent[h] >= 0 else 0.0) for h in heads}
    stab = {int(h): 0.0 for h in heads}
    for p in np.flatnonzero(a >= 0):
        h = int(cl[a[p]])
        stab[h] += lam[p] - birth[h]
    for s in np.flatnonzero(split):
        h = int(cl[s])
        stab[h] += float(nsize[s]) * (lam_node[s] - birth[h])
    pc = {int(h): (int(cl[parent[h]]) if parent[h] >= 0 else -1) for h in heads}
    kids = {int(h): [] for h in heads}
    S, win, margin = {}, {}, np.inf
    for h in heads.tolist():  # ascending: children before parents
        if not kids[h]:
            S[h], win[h] = stab[h], True
        else:
            assert len(kids[h]) == 2
            below = S[kids[h][0]] + S[kids[h][1]]
            S[h], win[h] = max(stab[h], below), stab[h] >= below
            if max(stab[h], below) > 0:
                margin = min(margin, abs(stab[h] - below) / max(stab[h], below))
        if pc[h] >= 0:
            kids[pc[h]].append(h)
        else:
            win[h] = False
    chosen = {}
    for h in heads[::-1].tolist():
        up = chosen[pc[h]] if pc[h] >= 0 else -1
        chosen[h] = up if up >= 0 else (h if win[h] else -1)
    raw = np.array([chosen[int(cl[a[p]])] if a[p] >= 0 else -1 for p in range(n)], np.int64)
    out = np.full(n, -1, np.int32)
    seen = {}
    for p in range(n):
        if raw[p] >= 0:
            out[p] = seen.setdefault(int(raw[p]), len(seen))
    return {"labels": out, "lam": lam, "clusters": len(seen), "noise": int((out < 0).sum()), "condensed_clusters": len(heads), "stability": stab,
            "margin": float(margin), "dendrogram": d}


def rows_of(names, ids):
    """Names (ids, or rows where ids is None) back to rows."""
    if ids is None:
        return np.asarray(names, np.int64)
    inv = {int(i): r for r, i in enumerate(np.asarray(ids).tolist())}
    return np.array([inv[int(x)] for x in np.asarray(names).tolist()], np.int64)


# the sets and parameters of the GPU tests: emst_spec's uniform, mixture, planar, duplicates (w = 0), nan and far sets
SETS = ("uniform", "mixture", "planar", "duplicates", "nan", "far")
GPU_CASES = [(name, min_samples) for name in SETS for min_samples in (1, 6)]
MIN_CLUSTER_SIZES = (2, 5, 25)

_cache = {}


def hdbscan_case(name, min_cluster_size, min_samples, ids=None):
    """The spec's answer for the set emst_spec.point_set / case `name`: the core distances, tknnEmst's records (by name), and
    labels() of them with the names mapped back to rows.  Computed once and shared (do not write to them)."""
    import emst_spec as em

    key = (name, min_cluster_size, min_samples, None if ids is None else "ids")
    if key not in _cache:
        P = points(name)
        tkey = (name, min_samples, None if ids is None else "ids")
        if tkey not in _cache:
            core = em.core_distances(P, min_samples, ids=ids) if min_samples > 1 else None
            _cache[tkey] = (core, em.mst(P, core, ids))
        core, tree = _cache[tkey]
        want = labels(len(P), rows_of(tree["u"], ids), rows_of(tree["v"], ids), tree["w"], min_cluster_size)
        want.update(core=core, tree=tree, P=P)
        _cache[key] = want
    return _cache[key]


def points(name):
    import emst_spec as em

    if name in em.SET_NAMES:
        return em.point_set(name)
    if name == "blobs":  # six blobs of unequal spread: clusters at several levels of the condensed tree
        rng = np.random.default_rng(91)
        c = rng.random((6, 3), dtype=np.float32)
        s = np.float32([0.01, 0.02, 0.03, 0.015, 0.04, 0.025])
        k = rng.integers(0, 6, 1800)
        return np.ascontiguousarray((c[k] + rng.standard_normal((1800, 3), dtype=np.float32) * s[k, None]).astype(np.float32))
    return {"duplicates": em.duplicates_case, "nan": em.nan_case, "far": em.far_case}[name]()


# ---- trees for tknnLinkage --------------------------------------------------------------------------------------------------------
def tree(kind, n, seed=0, ranks="random"):
    """(u, v) of a tree over n vertices, the records in rank order: a path, a star, a caterpillar (a spine of n // 2 vertices,
    every other vertex a leg) or a random recursive tree; ranks random, or `along` (the rank grows with the position: one long
    chain of pointers in the first round)."""
    rng = np.random.default_rng(seed)
    i = np.arange(1, n)
    if kind == "path":
        a = i - 1
    elif kind == "star":
        a = np.zeros(n - 1, np.int64)
    elif kind == "caterpillar":
        spine = max(n // 2, 1)
        a = np.where(i < spine, i - 1, rng.integers(0, spine, n - 1))
    else:
        a = (rng.random(n - 1) * i).astype(np.int64)
    order = rng.permutation(n - 1) if ranks == "random" else np.arange(n - 1)
    relabel = rng.permutation(n) if ranks == "random" else np.arange(n)
    a, b = relabel[a[order]], relabel[i[order]]
    return np.minimum(a, b).astype(np.int32), np.maximum(a, b).astype(np.int32)
