"""One table of scenarios, one per public call that takes a built (or bare) engine, for the tests of what a call may find in the
engine when it starts (tests/test_engine_state_gpu.py).  No tests here.

A scenario names its call (the key of NOT_REPRODUCIBLE entries), the forced-fallback variable of that call where it has one, which
trees it applies to, `run(eng, tree)` -- the call on an engine that holds the tree, returning the wrapper's result -- and
`check(tree, flat)`, the family's own comparison with its CPU spec (the spec modules are called; no tolerance is restated here).
`flat(result)` turns a result into a flat dict of numpy arrays: every output tensor and every field of the info records but the
times.  The trees are the spec modules' sets, reduced to what every scenario needs of them:

  n1025    reduce_spec n1025     the last leaf block holds one point; two pyramid levels
  n17ids   reduce_spec n17       no pyramid: every call's lane kernel; ids a permutation of the rows
  nan700   reduce_spec nan       45 points and a query with NaN coordinates
  n1025b3  reduce_spec n1025     three batches in one tree
  n1       reduce_spec n1        one point: no internal node
  n4097    uniform               257 leaf blocks, the last of one point; five boxes on the second pyramid level

`<tree>q<m>` (n1025q1, n1025q63, n1025q65, n1025b3q65) is the tree with the first m of its queries: one query, one short of a wave,
one more than a wave.  The CPU references are cached by the tree's name, so a variant has its own.

TABLE is what tests/test_engine_state_gpu.py runs.  GUARDED_ONLY holds the scenarios that only tests/test_output_bounds_gpu.py
reads (they would lengthen the other file's chain): the calls whose state files bring their own point sets, the row-writing calls
at the register lists' capacities, and the calls that document a region they do not write.
"""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_spec as bs  # noqa: E402
import dbscan_query_spec as dq  # noqa: E402
import emst_spec as em  # noqa: E402
import fps_spec as fs  # noqa: E402
import halo_spec as hl  # noqa: E402
import hdbscan_spec as hs  # noqa: E402
import knn_spec as kn  # noqa: E402
import nms_spec as ns  # noqa: E402
import pca_spec as ps  # noqa: E402
import periodic_spec as pp  # noqa: E402
import query_spec as qs  # noqa: E402
import radius_knn_spec as rk  # noqa: E402
import radius_spec as rs  # noqa: E402
import reduce_spec as rd  # noqa: E402
import tile_sets  # noqa: E402

import oracle  # noqa: E402
from oracle.trueknn_numpy import trueknn_numpy  # noqa: E402
from owlraytracing_amd import _lib, datasets  # noqa: E402

K_SMALL, K_BIG = 5, 100  # register lists; the lists in memory (trueknn_bigk)
MIN_PTS = 3
MCS, MIN_SAMPLES = 5, 6
MARGIN = 1e-6  # tests/test_hdbscan_expectations.py: the excess-of-mass margin above which the labels do not depend on the order of a sum


# ---- the trees ---------------------------------------------------------------------------------------------------------------------
def _variant(name):
    """The tree `<base>q<m>`: the base tree with the first m of its queries."""
    base, m = name.rsplit("q", 1)
    t = dict(tree(base))
    m = int(m)
    assert 0 < m < len(t["Q"])
    t["name"] = name
    t["Q"] = np.ascontiguousarray(t["Q"][:m])
    t["Qf"] = np.ascontiguousarray(t["Q"][~np.isnan(t["Q"]).any(axis=1)])
    t["qbatch"] = np.ascontiguousarray(t["qbatch"][:m])
    for a in (t["Q"], t["Qf"], t["qbatch"]):
        a.setflags(write=False)
    return t


def _tree(name):
    if name == "own":  # the scenario brings its own set and builds it (GUARDED_ONLY)
        return {"name": "own", "n": 0, "nan": False, "batch": None, "ids": None}
    if name.rsplit("q", 1)[-1].isdigit() and "q" in name:
        return _variant(name)
    ids = batch = None
    if name == "n4097":
        P = datasets.uniform3d(4097, seed=97)
        Q = np.random.default_rng(98).random((96, 3), dtype=np.float32)
        Q[7] = [0.5, np.nan, 0.5]
        r, eps = 0.1, 0.05
    else:
        c = rd.case({"n1025": "n1025", "n17ids": "n17", "nan700": "nan", "n1025b3": "n1025", "n1": "n1"}[name])
        P, Q, r = c["P"], c["Q"], float(c["radii"]["mid"])
        eps = {"n1025": 0.08, "n17ids": 0.35, "nan700": 0.09, "n1025b3": 0.08, "n1": 0.1}[name]
        if name == "n17ids":
            ids = np.random.default_rng(17).permutation(17).astype(np.int32)
        if name == "n1025b3":
            batch = np.random.default_rng(18).integers(0, 3, len(P)).astype(np.int32)
    n = len(P)
    clean = ~np.isnan(P).any(axis=1)
    t = {"name": name, "P": np.ascontiguousarray(P, np.float32), "Q": np.ascontiguousarray(Q, np.float32), "ids": ids, "batch": batch,
         "num_batches": None if batch is None else 3, "n": n, "r": np.float32(r), "eps": np.float32(eps), "nan": not clean.all(),
         "r0": np.float32(datasets.start_radius(max(n, 2), K_SMALL)) if n > 64 else np.float32(0.1), "values": rd.values_for(n, seed=n)}
    t["Qf"] = np.ascontiguousarray(t["Q"][~np.isnan(t["Q"]).any(axis=1)])  # for the calls whose NaN queries never finish
    t["names"] = np.arange(n, dtype=np.int64) if ids is None else ids.astype(np.int64)
    t["qbatch"] = np.random.default_rng(19).integers(0, 3, len(Q)).astype(np.int32)
    t["qbatch"][-1] = 5  # a label no batch has
    for a in t.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


TREE_NAMES = ("n4097", "n17ids", "n1025b3", "n1", "n1025", "nan700")
CHAIN = ("n4097", "n17ids", "n1025b3", "n1", "n1025")  # the builds of the chain, in order
_cache = {}


def tree(name):
    if ("tree", name) not in _cache:
        _cache[("tree", name)] = _tree(name)
    return _cache[("tree", name)]


def shared(key, make):
    """A CPU reference, computed once and shared (do not write to it)."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def build(eng, t):
    eng.build(np.array(t["P"]), ids=None if t["ids"] is None else np.array(t["ids"]), batch=None if t["batch"] is None else np.array(t["batch"]),
              num_batches=t["num_batches"])


# ---- results -----------------------------------------------------------------------------------------------------------------------
def flat(result, prefix=""):
    """Every tensor and array of a wrapper's result, every number of its info records but the times, as numpy arrays by name."""
    out = {}
    for name, v in result.items():
        if isinstance(v, dict):
            out.update(flat(v, prefix + name + "."))
        elif v is None or name.endswith("_ms"):
            continue
        elif hasattr(v, "cpu"):
            out[prefix + name] = v.cpu().numpy().copy()
        elif isinstance(v, np.ndarray):
            out[prefix + name] = v.copy()
        elif isinstance(v, (list, tuple)):
            out[prefix + name] = np.asarray(v)
        else:
            out[prefix + name] = np.asarray([v])
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind == "f" else a


def differing(got, want, skip=()):
    """The names of the arrays that are not the same bit for bit (or are missing on one side), `skip` left out."""
    names = sorted((set(got) | set(want)) - set(skip))
    return [f for f in names if f not in got or f not in want or got[f].shape != want[f].shape or got[f].dtype != want[f].dtype
            or not np.array_equal(bits(got[f]), bits(want[f]))]


# ---- solve, repair, query ------------------------------------------------------------------------------------------------------------
def _solve_k(t, big, k=None):
    return K_BIG if big else min(K_SMALL if k is None else k, t["n"] - 1)


def _global(t):
    """(G, rows): the set with every point at the position its name says, and the positions of the tree's rows."""
    G = np.empty_like(t["P"])
    G[t["names"]] = t["P"]
    return G, t["names"]


def _solve(kernel, big=False, levels=False, k=None):
    want_k = k

    def run(eng, t):
        return eng.solve(_solve_k(t, big, want_k), float(t["r0"]), kernel=kernel, want_levels=levels)

    def check(t, f):
        k = _solve_k(t, big, want_k)
        G, rows = _global(t)
        ref = shared(("solve", t["name"], k), lambda: oracle.trueknn(G, k, float(t["r0"])))
        assert np.array_equal(f["idx"], ref["idx"][rows]) and np.array_equal(bits(f["dist"]), bits(ref["dist"][rows])), "rows differ from the replay"
        assert np.array_equal(f["intersections"], ref["intersections"][rows]) and f["info.rounds"][0] == ref["rounds"]
        assert f["info.unfinished"][0] == 0 and f["info.tie_rows_left"][0] == 0
        if levels:
            lv = shared(("levels", t["name"], k), lambda: trueknn_numpy(G, k, float(t["r0"]))["level"])
            assert np.array_equal(f["levels"], lv[rows])
    return run, check


def _repair():
    def run(eng, t):
        k = _solve_k(t, False)
        r = eng.solve(k, float(t["r0"]), want_levels=True)
        out = {"idx": r["idx"], "dist": r["dist"], "levels": r["levels"]}
        out["repaired"] = eng.repair_exact(out, k, float(t["r0"]))
        return out

    def check(t, f):
        want = shared(("self", t["name"], _solve_k(t, False)), lambda: kn.self_rows(t["P"], _solve_k(t, False), ids=t["ids"]))
        assert np.array_equal(f["idx"], want["idx"]) and np.array_equal(bits(f["dist"]), bits(want["dist"]))
    return run, check


def _query(k=K_SMALL):
    want_k = k

    def run(eng, t):
        return eng.query(np.array(t["Qf"]), min(want_k, t["n"]), float(t["r0"]), want_levels=True)

    def check(t, f):
        k = min(want_k, t["n"])
        want = shared(("query", t["name"], k), lambda: qs.query_rows(t["P"], t["Qf"], [k], float(t["r0"]), ids=t["ids"])[k])
        for name in ("idx", "intersections", "levels"):
            assert np.array_equal(f[name], want[name]), name
        assert np.array_equal(bits(f["dist"]), bits(want["dist"]))
        for name in ("rounds", "total_intersections", "total_active_rounds", "unfinished"):
            assert f["info." + name][0] == want[name], name
    return run, check


# ---- RT-DBSCAN -----------------------------------------------------------------------------------------------------------------------
def _db_ref(t):
    return shared(("dbscan", t["name"]), lambda: oracle.dbscan(t["P"], float(t["eps"]), MIN_PTS))


def _core_label(t):
    ref = _db_ref(t)
    return np.where(ref["core"], ref["labels"], -1).astype(np.int32)


def _dbscan():
    def run(eng, t):
        return eng.dbscan(float(t["eps"]), MIN_PTS, want_counts=True)

    def check(t, f):
        ref = _db_ref(t)
        assert np.array_equal(f["labels"], ref["labels"]) and np.array_equal(f["core"], ref["core"]) and np.array_equal(f["counts"], ref["counts"])
        assert f["info.clusters"][0] == ref["clusters"]
    return run, check


def _dbscan_auto():
    def run(eng, t):
        return eng.dbscan_auto(float(t["eps"]) / 4, MIN_PTS, max_noise=0.2)

    def check(t, f):
        ref = shared(("dbscan_auto", t["name"]), lambda: oracle.dbscan_auto(t["P"], float(t["eps"]) / 4, MIN_PTS, max_noise=0.2))
        assert np.array_equal(f["labels"], ref["labels"]) and np.array_equal(f["core"], ref["core"])
        assert (f["info.rounds"][0], f["info.noise"][0], f["info.clusters"][0]) == (ref["rounds"], ref["noise"], ref["clusters"])
        assert np.float32(f["info.eps"][0]) == np.float32(ref["eps"])
    return run, check


def _dbscan_noise():
    def run(eng, t):
        return eng.dbscan_noise(float(t["eps"]), MIN_PTS)

    def check(t, f):
        ref = _db_ref(t)
        assert np.array_equal(f["noise"], ref["labels"] < 0) and f["count"][0] == (ref["labels"] < 0).sum()
    return run, check


def _dbscan_assign():
    def run(eng, t):
        return {"labels": eng.dbscan_assign(float(t["eps"]), _core_label(t))}

    def check(t, f):
        assert np.array_equal(f["labels"], _db_ref(t)["labels"]), "a border point takes the smallest label among its core neighbours"
    return run, check


def _dbscan_query():
    # (at the eps of the clustering: core points within eps of each other must carry the same label)
    def run(eng, t):
        return eng.dbscan_query(np.array(t["Q"]), float(t["eps"]), _core_label(t), want_counts=True)

    def check(t, f):
        labels, counts = shared(("dbscan_query", t["name"]), lambda: dq.query_labels(t["P"], _core_label(t), float(t["eps"]), t["Q"]))
        assert np.array_equal(f["labels"], labels) and np.array_equal(f["counts"], counts)
    return run, check


# ---- neighbour lists ---------------------------------------------------------------------------------------------------------------
def _radius_query(sort):
    def run(eng, t):
        r = eng.radius_query(np.array(t["Q"]), float(t["r"]), sort=sort)
        if not sort:  # the order inside an unsorted row is the order of the kernel's atomics: each row put in (distance, index) order here
            off, idx, dist = (r[name].cpu().numpy() for name in ("offsets", "idx", "dist"))
            row = np.repeat(np.arange(len(off) - 1), np.diff(off))
            order = np.lexsort((idx, dist.view(np.uint32), row))
            r["idx"], r["dist"] = idx[order], dist[order]
        return r

    def check(t, f):
        want = shared(("radius", t["name"]), lambda: rs.radius_rows(t["P"], t["Q"], t["r"], ids=t["ids"]))
        assert np.array_equal(f["offsets"], want["offsets"]) and f["info.total"][0] == f["count_info.total"][0] == want["lengths"].sum()
        assert np.array_equal(f["idx"], want["idx"]) and np.array_equal(bits(f["dist"]), bits(want["dist"]))
    return run, check


def _rows_equal(f, want):
    assert np.array_equal(f["idx"], want["idx"]) and np.array_equal(bits(f["dist"]), bits(want["dist"])) and np.array_equal(f["counts"], want["counts"])
    assert f["info.total"][0] == want["counts"].sum()


def _skip(t):
    """Every third query leaves out the point of its own number (by name), the others nothing."""
    m = len(t["Q"])
    return np.where(np.arange(m) % 3 == 0, t["names"][np.arange(m) % t["n"]], -1).astype(np.int32)


def _radius_knn(k=8):
    def run(eng, t):
        return eng.radius_knn(np.array(t["Q"]), k, radius=float(t["r"]), skip_ids=_skip(t))

    def check(t, f):
        _rows_equal(f, shared(("radius_knn", t["name"], k), lambda: rk.knn_rows(t["P"], t["Q"], k, radius=t["r"], skip=_skip(t), ids=t["ids"])))
    return run, check


def _knn(own, k=8):
    def run(eng, t):
        return eng.knn(None if own else np.array(t["Q"]), k=k)

    def check(t, f):
        _rows_equal(f, shared(("knn", own, t["name"], k), lambda: kn.self_rows(t["P"], k, ids=t["ids"]) if own else kn.knn_rows(t["P"], t["Q"], k, ids=t["ids"])))
    return run, check


CELL = ((0.0, 0.0, 0.0), (1.0, 1.0, 0.0))  # x and y periodic, z open: every set here lies in [0, 1)


def _periodic_knn(k=8):
    def run(eng, t):
        return eng.periodic_knn(np.array(t["Q"]), k=k, lo=CELL[0], period=CELL[1], radius=float(t["r"]))

    def check(t, f):
        _rows_equal(f, shared(("periodic", t["name"], k), lambda: pp.knn_rows(t["P"], t["Q"], k, CELL[0], CELL[1], radius=t["r"], ids=t["ids"])))
    return run, check


def _batch_knn(k=8):
    def run(eng, t):
        return eng.batch_knn(np.array(t["Q"]), k=k, batch=np.array(t["qbatch"]))

    def check(t, f):
        _rows_equal(f, shared(("batch", t["name"], k), lambda: bs.knn_rows(t["P"], t["batch"], t["Q"], t["qbatch"], k, ids=t["ids"])))
    return run, check


# ---- spanning trees, dendrograms, HDBSCAN ------------------------------------------------------------------------------------------------
def _emst(mutual):
    def core(t):
        return shared(("core", t["name"]), lambda: em.core_distances(t["P"], MIN_SAMPLES, ids=t["ids"])) if mutual else None

    def run(eng, t):
        return eng.emst(core_dist=None if not mutual else np.array(core(t)), want_components=mutual)

    def check(t, f):
        want = shared(("emst", mutual, t["name"]), lambda: em.mst(t["P"], core(t), t["ids"]))
        assert (f["edges"][0], f["info.edges"][0], f["info.components"][0], f["info.excluded"][0]) == (want["edges"], want["edges"], want["components"], want["excluded"])
        assert np.array_equal(f["u"], want["u"]) and np.array_equal(f["v"], want["v"]) and np.array_equal(bits(f["w"]), bits(want["w"]))
        assert not mutual or np.array_equal(f["components"], want["component"])
        assert 0 <= f["info.rounds"][0] <= em.round_bound(t["n"])
    return run, check


def forest(t):
    """(u, v, w, the spec's labels) of a random tree over the tree's n vertices in rank order, the weights ascending: the first seed whose
    excess-of-mass decisions have the margin the labels need."""
    def make():
        n = t["n"]
        if n == 1:
            u = v = np.zeros(0, np.int32)
            return u, v, np.zeros(0, np.float32), hs.labels(1, u, v, np.zeros(0, np.float32), MCS)
        for seed in range(n, n + 50):
            u, v = hs.tree("random", n, seed=seed)
            w = np.sort(np.random.default_rng(seed).random(n - 1, dtype=np.float32) + np.float32(0.01))
            want = hs.labels(n, u, v, w, MCS)
            if want["margin"] >= MARGIN:
                return u, v, w, want
        raise AssertionError("no forest with a margin")
    return shared(("forest", t["name"]), make)


def _same_dendrogram(f, d):
    for name in ("parent", "left", "right", "size"):
        assert np.array_equal(f[name], d[name]), name


def _linkage(max_rounds):
    def run(eng, t):
        u, v, w, _ = forest(t)
        return eng.linkage(u, v, n=t["n"], max_rounds=max_rounds)

    def check(t, f):
        u, v, _, _ = forest(t)
        _same_dendrogram(f, hs.dendrogram(t["n"], u, v))
        assert f["info.roots"][0] == t["n"] - len(u) and f["info.absorbed"][0] + f["info.host_edges"][0] == len(u)
        if max_rounds == 1 and t["n"] > 64:
            assert f["info.host_edges"][0] == hs.contraction(t["n"], u, v, max_rounds=1)["host_edges"] > 0, "the host finishes it"
    return run, check


def _check_labels(f, want, n):
    assert np.array_equal(f["labels"], want["labels"])
    assert (f["info.clusters"][0], f["info.noise"][0], f["info.condensed_clusters"][0]) == (want["clusters"], want["noise"], want["condensed_clusters"])
    assert np.array_equal(bits(f["lam"]), bits(want["lam"]))
    _same_dendrogram(f, want["dendrogram"])
    heads = np.array(sorted(want["stability"]), np.int64)
    ref = np.array([want["stability"][h] for h in heads.tolist()])
    assert np.array_equal(np.flatnonzero(f["stability"]), heads[ref > 0] - n)
    worst = float(np.max(np.abs(f["stability"][heads - n] - ref) / np.maximum(ref, np.finfo(np.float64).tiny), initial=0.0))
    assert worst <= 1e-9, worst  # tests/test_hdbscan_gpu.py: the order of the additions is free


def _hdbscan_labels():
    def run(eng, t):
        u, v, w, _ = forest(t)
        return eng.hdbscan_labels(u, v, w, n=t["n"], min_cluster_size=MCS, want_linkage=True, want_lambda=True, want_stability=True)

    def check(t, f):
        _check_labels(f, forest(t)[3], t["n"])
    return run, check


def _hdbscan():
    def run(eng, t):
        return eng.hdbscan(MCS, MIN_SAMPLES, want_tree=True, want_linkage=True, want_lambda=True, want_core_dist=True, want_stability=True)

    def check(t, f):
        def make():
            core = em.core_distances(t["P"], MIN_SAMPLES, ids=t["ids"])
            rec = em.mst(t["P"], core, t["ids"])
            want = hs.labels(t["n"], hs.rows_of(rec["u"], t["ids"]), hs.rows_of(rec["v"], t["ids"]), rec["w"], MCS)
            want.update(core=core, tree=rec)
            return want
        want = shared(("hdbscan", t["name"]), make)
        assert want["margin"] >= MARGIN, "the set's labels depend on the order of a sum: take another set"
        rec = want["tree"]
        assert (f["edges"][0], f["info.excluded"][0]) == (rec["edges"], rec["excluded"])
        assert np.array_equal(f["u"], rec["u"]) and np.array_equal(f["v"], rec["v"]) and np.array_equal(bits(f["w"]), bits(rec["w"]))
        assert np.array_equal(bits(f["core_dist"]), bits(want["core"]))
        _check_labels(f, want, t["n"])
    return run, check


# ---- sampling, suppression ---------------------------------------------------------------------------------------------------------
def _fps():
    def run(eng, t):
        return eng.fps(num_samples=20)

    def check(t, f):
        want = shared(("fps", t["name"]), lambda: fs.brute(t["P"], 20, batch=t["batch"], num_batches=t["num_batches"], ids=t["ids"]))
        assert np.array_equal(f["counts"], want["counts"]) and np.array_equal(f["idx"], want["idx"]) and np.array_equal(bits(f["dist"]), bits(want["dist"]))
        assert f["info.samples"][0] == want["counts"].sum() and f["info.bad_starts"][0] == 0
    return run, check


def _scores(t):
    s = np.random.default_rng(23).random(t["n"], dtype=np.float32)
    s[:: 9] = s[1:: 9][: len(s[:: 9])] if t["n"] > 9 else s[:: 9]  # equal scores: the name decides
    return s


def _nms(scored, apart=False):
    """apart: a radius below every distance between two points -- every point is kept in the first round, so the call takes exactly
    one round whatever the order of its walks (the longest chain of dominators has one link)."""
    def radius(t):
        return 1e-4 if apart else float(t["r"]) / 2

    def args(t):
        return dict(scores=_scores(t) if scored else None, batch=t["batch"], num_batches=t["num_batches"], ids=t["ids"])

    def run(eng, t):
        return eng.radius_nms(radius(t), scores=_scores(t) if scored else None, want_cover=True)

    def check(t, f):
        want = shared(("nms", scored, apart, t["name"]), lambda: ns.brute(t["P"], radius(t), **args(t)))
        deepest = shared(("nms_depth", scored, apart, t["name"]), lambda: int(ns.depth(t["P"], radius(t), **args(t)).max()))
        assert np.array_equal(f["counts"], want["counts"]) and np.array_equal(f["keep"], want["keep"]) and np.array_equal(f["cover"], want["cover"])
        assert np.array_equal(f["idx"], t["names"][want["keep"]])
        assert f["info.kept"][0] == want["counts"].sum() and f["info.eligible"][0] == want["eligible"] and f["info.bad_scores"][0] == want["bad_scores"]
        assert not apart or deepest == 1
        assert 1 <= f["info.rounds"][0] <= max(deepest, 1), "more rounds than the longest chain of dominators has links"
    return run, check


# ---- sums and moments over a neighbourhood -------------------------------------------------------------------------------------------
def _reduce(weight, C, own):
    def run(eng, t):
        return eng.radius_reduce(float(t["r"]), queries=None if own else np.array(t["Q"]), values=None if C == 0 else np.ascontiguousarray(t["values"][:, :C]),
                                 weight=weight, bandwidth=rd.bandwidth(t["r"]), skip_self=own)

    def check(t, f):
        mem = shared(("reduce_rows", own, t["name"]), lambda: rd.members(t["P"], None if own else t["Q"], t["r"], skip_self=own))
        want = shared(("reduce", weight, own, t["name"]), lambda: rd.sums(mem, t["values"], weight, t["r"], rd.bandwidth(t["r"])))
        got = {"counts": f["counts"], "wsum": f["wsum"], "out": f.get("out")}
        rd.compare(got, want, weight, t["r"], rd.bandwidth(t["r"]), channels=C)
        assert f["info.total"][0] == want["counts"].sum() and f["info.max_row"][0] == (want["counts"].max() if len(want["counts"]) else 0)
    return run, check


def _pca(hood, own, k=None):
    """hood: (whether the radius bounds the neighbourhood, the k that does or None); `k` replaces the hood's in the k mode."""
    hood = hood if k is None or hood[1] is None else (hood[0], k)
    radius, k = hood

    def run(eng, t):
        return eng.local_pca(radius=None if radius is None else float(t["r"]), k=k, queries=None if own else np.array(t["Q"]))

    def check(t, f):
        import test_pca_gpu  # the family's comparison

        def make():
            Q = None if own else t["Q"]
            return ps.want(t["P"], Q, ps.members(t["P"], Q, radius=None if radius is None else t["r"], k=k, ids=t["ids"]))
        w = shared(("pca", hood, own, t["name"]), make)
        got = {name: f[name] for name in ps.OUTPUTS}
        got["info"] = {name: (1.0 if name.endswith("_ms") else int(f["info." + name][0])) for name in ("total", "max_row", "degenerate_rows", "fallback_items",
                                                                                                   "solve_ms", "walk_ms", "finish_ms")}
        test_pca_gpu.check(got, w, t["P"] if own else t["Q"], what="%s %s" % (t["name"], hood))
    return run, check


# ---- the tile surface: halo selection, a halo tree and the phase solves ----------------------------------------------------------------
def _boxes(t):
    """Five closed boxes of two peers (and one of a peer that gets nothing) around points of the set."""
    rng = np.random.default_rng(29)
    clean = t["P"][~np.isnan(t["P"]).any(axis=1)]
    centres = clean[rng.integers(0, len(clean), 5)]
    half = np.float32([0.3, 0.2, 0.25, 0.15, 1e-4])[:, None]
    return np.concatenate([centres - half, centres + half], axis=1).astype(np.float32), np.int32([0, 1, 0, 1, 2]), 4


def _sorted_rows(rows, starts, counts):
    """Wire rows with every peer's segment in the order of the ids: the order inside a segment is the order of the kernel's atomics."""
    out = []
    for s, c in zip(starts, counts):
        seg = rows[s:s + c]
        out.append(seg[np.argsort(seg[:, 3].view(np.int32), kind="stable")])
    return np.concatenate(out) if out else rows[:0]


def _check_select(t, f, counts):
    boxes, peer, npeers = _boxes(t)
    lists, _ = hl.select(t["P"], t["names"].astype(np.int32), boxes, peer, npeers)
    assert [int(c) for c in counts] == [len(x) for x in lists]
    at = 0
    for p in range(npeers):
        got = f["rows"][at:at + len(lists[p])]
        assert np.array_equal(got[:, 3].view(np.int32), lists[p]), "peer %d" % p
        row = hl.row_of_id(t["names"].astype(np.int32))
        assert np.array_equal(bits(got[:, :3]), bits(t["P"][row(lists[p])].reshape(-1, 3)))
        at += len(lists[p])


def _halo_select():
    def run(eng, t):
        boxes, peer, npeers = _boxes(t)
        rows, counts = eng.halo_select(boxes, peer, npeers)
        rows = rows.cpu().numpy()
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        return {"rows": _sorted_rows(rows, starts, counts), "counts": np.asarray(counts, np.int64)}

    def check(t, f):
        _check_select(t, f, f["counts"])
    return run, check


def _halo_select_fixed():
    def run(eng, t):
        boxes, peer, npeers = _boxes(t)
        caps = [t["n"]] * npeers  # every peer's rows fit
        messages, starts, counts = eng.halo_select_fixed(boxes, peer, npeers, caps)
        counts = counts.cpu().numpy()
        return {"rows": _sorted_rows(messages.cpu().numpy(), [s + 1 for s in starts], counts), "counts": counts}

    def check(t, f):
        _check_select(t, f, f["counts"])
    return run, check


def _neighbour_tile(t):
    """The points of a second tile beside the tree's (the set mirrored at x = 1), named from n on."""
    rest = np.array(t["P"])
    rest[:, 0] = np.float32(2.0) - rest[:, 0]
    return np.ascontiguousarray(rest), (t["n"] + np.arange(t["n"])).astype(np.int32)


def _phase_layout(t):
    def make():
        k = _solve_k(t, False)
        G, own = _global(t)
        rest_xyz, rest = _neighbour_tile(t)
        G = np.concatenate([G, rest_xyz])
        r0 = float(t["r0"])
        lv = trueknn_numpy(G, k, r0)["level"]
        cap = tile_sets.phase_cap(lv)
        lay = tile_sets.phases(G, own.astype(np.int32), rest, r0, cap)
        return {"G": G, "own": own, "lv": lv, "cap": cap, "lay": lay, "ref": oracle.trueknn(G, k, r0), "k": k}
    return shared(("phases", t["name"]), make)


def _phases(poison_between=False):
    """tknnHaloSelect's count pass marks the boundary queries, a phase-1 solve serves the interior ones in the own tree, tknnSetHalo
    brings the neighbour's points within reach, a phase-2 solve serves the boundary ones.  What the second solve takes from the first
    is the boundary marks and the caller's rows and levels, not the per-slot solve state: poison_between fills
    that too, with everything else, between the two."""
    def run(eng, t):
        import torch

        from owlraytracing_amd import _debug_lib

        L = _phase_layout(t)
        k, n = L["k"], t["n"]
        eng.set_halo(None, None)
        _, counts = eng.halo_select(L["lay"]["peer_box"][None, :], [1], 2)

        def sentinel(nbytes, dtype, shape):
            return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=eng.device).view(dtype).view(shape)
        out = {"idx": sentinel(n * k * 4, torch.int32, (n, k)), "dist": sentinel(n * k * 4, torch.float32, (n, k)),
               "intersections": sentinel(n * 8, torch.int64, (n,)), "levels": sentinel(n * 4, torch.int32, (n,))}
        kw = dict(kernel=_lib.KERNEL_TEAM, max_rounds=L["cap"] + 1, allow_unfinished=True, want_levels=True)
        r1 = eng.solve(k, float(t["r0"]), out=out, phase=1, **kw)
        first = {name: out[name].clone() for name in out}
        near = L["lay"]["near"]
        if poison_between:
            _debug_lib.poison(eng, _debug_lib.POISON_ALL, 0x5A)
        eng.set_halo(L["G"][near], near)
        if poison_between:
            _debug_lib.poison(eng, _debug_lib.POISON_ALL, 0xFF)
        try:
            r2 = eng.solve(k, float(t["r0"]), out=out, phase=2, **kw)
        finally:
            eng.set_halo(None, None)
        res = {"phase1." + name: v for name, v in first.items()}
        res.update({"phase2." + name: out[name] for name in ("idx", "dist", "intersections", "levels")})
        res.update({"counts": np.asarray(counts), "info1": r1["info"], "info2": r2["info"]})
        return res

    def check(t, f):
        L = _phase_layout(t)
        own, lv, cap, ref = L["own"], L["lv"][L["own"]], L["cap"], L["ref"]
        boundary = L["lay"]["boundary"]
        assert f["counts"][1] == boundary.sum()
        capped = np.where(lv <= cap, lv, -1)
        assert np.array_equal(f["phase1.levels"], np.where(~boundary, capped, -1)) and np.array_equal(f["phase2.levels"], capped)
        for phase, fin in (("phase1.", ~boundary & (lv <= cap)), ("phase2.", lv <= cap)):
            assert np.array_equal(f[phase + "idx"][fin], ref["idx"][own][fin]), phase
            assert np.array_equal(bits(f[phase + "dist"][fin]), bits(ref["dist"][own][fin])), phase
            assert np.array_equal(f[phase + "intersections"][fin], ref["intersections"][own][fin]), phase
        assert f["info1.unfinished"][0] == (~boundary & (lv > cap)).sum() and f["info2.unfinished"][0] == (boundary & (lv > cap)).sum()
    return run, check


# ---- what a batched build made ---------------------------------------------------------------------------------------------------------
def _batch_layout():
    def run(eng, t):
        return eng.batch_layout()

    def check(t, f):
        clean = ~np.isnan(t["P"]).any(axis=1)
        sizes = np.bincount(t["batch"][clean], minlength=t["num_batches"])
        assert f["num_batches"][0] == t["num_batches"] and np.array_equal(f["starts"], np.concatenate([[0], np.cumsum(sizes)]))
    return run, check


# ---- rows that a call documents as not written -------------------------------------------------------------------------------------------
def _level_cap(t, k):
    """(levels of the replay by row, the last level a capped solve still serves): one below the deepest, so that some rows stay."""
    G, rows = _global(t)
    lv = shared(("levels", t["name"], k), lambda: trueknn_numpy(G, k, float(t["r0"]))["level"])[rows]
    return lv, int(lv.max()) - 1


def _solve_unfinished():
    def run(eng, t):
        k = _solve_k(t, False)
        return eng.solve(k, float(t["r0"]), kernel=_lib.KERNEL_TEAM, max_rounds=_level_cap(t, k)[1] + 1, allow_unfinished=True)

    def check(t, f):
        k = _solve_k(t, False)
        G, rows = _global(t)
        lv, cap = _level_cap(t, k)
        fin = lv <= cap
        assert 0 < fin.sum() < len(fin), "some rows finish and some do not"
        ref = shared(("solve", t["name"], k), lambda: oracle.trueknn(G, k, float(t["r0"])))
        assert np.array_equal(f["levels"], np.where(fin, lv, -1)) and f["info.unfinished"][0] == (~fin).sum()
        assert np.array_equal(f["idx"][fin], ref["idx"][rows][fin]) and np.array_equal(bits(f["dist"][fin]), bits(ref["dist"][rows][fin]))
        assert np.array_equal(f["intersections"][fin], ref["intersections"][rows][fin])
    return run, check


QUERY_ROUNDS = 2  # of the capped query: rows that need a third radius, and the NaN query, stay unfinished


def _query_unfinished():
    def run(eng, t):
        return eng.query(np.array(t["Q"]), min(K_SMALL, t["n"]), float(t["r0"]), max_rounds=QUERY_ROUNDS, allow_unfinished=True)

    def check(t, f):
        k = min(K_SMALL, t["n"])
        want = shared(("query_capped", t["name"]), lambda: qs.query_rows(t["P"], t["Q"], [k], float(t["r0"]), ids=t["ids"], max_rounds=QUERY_ROUNDS)[k])
        fin = want["levels"] >= 0
        assert 0 < fin.sum() < len(fin), "some rows finish and some do not"
        assert np.array_equal(f["levels"], want["levels"]) and f["info.unfinished"][0] == want["unfinished"]
        assert np.array_equal(f["idx"][fin], want["idx"][fin]) and np.array_equal(bits(f["dist"][fin]), bits(want["dist"][fin]))
        assert np.array_equal(f["intersections"][fin], want["intersections"][fin])
    return run, check


# ---- the calls whose state files bring their own sets: their runners and their comparisons ------------------------------------------------
def _mean_shift_modes(kernel, own=False):
    def run(eng, t):
        import test_meanshift_state_gpu as m

        P, S, Q, big = m.case()
        eng.build(P)
        return m.shift(eng, kernel, S, own=own)

    def check(t, f):
        info = f["info"]  # (iterations, walks, converged, empty, running, invalid): what that file's fresh results are held to
        if not own:
            assert info[0] >= 2 and info[1] < 1300 * info[0] and info[3] == 1 and info[5] == 1, "several passes, a shrinking list, an EMPTY and an INVALID seed"
        assert info[2] + info[3] + info[4] + info[5] == len(f["status"]) and f["status"].max() <= 3
    return run, check


def _mean_shift():
    """The clustering on top: tests/test_meanshift_gpu.py's comparison -- the merge and the labels are the spec's, applied to the
    device's own modes and scores, exactly."""
    import meanshift_spec as ms

    def run(eng, t):
        P, _ = ms.blobs()
        eng.build(np.array(P))
        return eng.mean_shift(ms.BLOB_KERNELS["flat"]["bandwidth"], points=np.array(P), max_iterations=10)

    def check(t, f):
        P, comp = ms.blobs()
        want = ms.merge_and_label(P, f["modes"], f["counts"], f["status"], f["counts"], ms.BLOB_KERNELS["flat"]["bandwidth"])
        assert np.array_equal(bits(f["centers"]), bits(want["centers"])) and np.array_equal(f["labels"], want["labels"])
        assert np.array_equal(bits(f["scores"]), bits(want["scores"])) and len(f["centers"]) > 0
    return run, check


FPFH_BY_SPEC = ("fpfh", "spfh")  # tests/test_fpfh_state_gpu.py's rule: the floats inside the bound of the spec, the rest bit for bit


def _fpfh():
    def run(eng, t):
        import fpfh_spec as fs
        import test_fpfh_state_gpu as m

        eng.build(np.array(fs.case(m.NAME)["P"]))
        return m.describe(eng)

    def check(t, f):
        import test_fpfh_state_gpu as m

        m.same(f, f, "against the spec")  # (the counts against themselves; what it adds is the floats against the spec's bound)
    return run, check


def _icp(method):
    def run(eng, t):
        import test_icp_state_gpu as m

        P, nrm, S, Q = m.case()
        eng.build(P)
        return m.icp(eng, method, nrm, S)

    def check(t, f):
        assert f["counts"][2] >= 2 and f["counts"][0] > 1000 and f["corr"][5] == -1, "that file's: several iterations, pairs, no partner for the NaN"
    return run, check


def _global_calls(prefix):
    """tests/test_global_state_gpu.py runs the two calls together, on an engine without a tree: the outputs of one of them."""
    def run(eng, t):
        import test_global_state_gpu as m

        return {k: v for k, v in m.both(eng).items() if k.startswith(prefix)}

    def check(t, f):
        import global_spec as gs
        import test_global_state_gpu as m

        A, B, scene = m.cases()
        if prefix == "match.":
            best, b1, b2 = gs.match(A, B)
            assert np.array_equal(f["match.best"], best) and np.array_equal(f["match.best_d2"], b1.view(np.int32))
        else:
            tr = gs.scene_trials(3)[1]  # tests/test_ransac_gpu.py: the statuses are the spec's, but for the trials it leaves open
            held = np.flatnonzero(~tr["excluded"])
            assert np.array_equal(f["ransac.trial_status"][:gs.TRIALS][held], tr["status"][held])
            assert f["ransac.mask"].sum() == f["ransac.info"][1] > 0
    return run, check


# ---- the table ---------------------------------------------------------------------------------------------------------------------
class Scenario:
    def __init__(self, name, call, fns, fallback=None, trees=("n1025", "n17ids", "nan700"), applies=None, bare=False, by_spec=(), k=None):
        """by_spec: the float outputs that the family's own file does not compare bit for bit but holds to the spec (the check).
        k: the row width, where the scenario was made for one (the guarded test's account of what it ran)."""
        self.name, self.call, (self.run, self.check), self.fallback, self.trees, self.bare = name, call, fns, fallback, trees, bare
        self._applies, self.by_spec, self.k = applies, tuple(by_spec), k

    def applies(self, t):
        return self._applies is None or bool(self._applies(t))


def _solvable(t):
    return t["n"] > K_SMALL and not t["nan"]


PLAIN = ("n1025", "n17ids")
RKNN = "TKNN_RADIUS_KNN_FORCE_FALLBACK"
TABLE = (
    Scenario("solve_lane", "solve", _solve(_lib.KERNEL_LANE), trees=PLAIN, applies=_solvable),
    Scenario("solve_wave", "solve", _solve(_lib.KERNEL_WAVE), trees=PLAIN, applies=_solvable),
    Scenario("solve_team", "solve", _solve(_lib.KERNEL_TEAM), trees=PLAIN, applies=_solvable),
    Scenario("solve_bigk", "solve", _solve(_lib.KERNEL_AUTO, big=True), trees=("n1025",), applies=lambda t: t["n"] > K_BIG and not t["nan"]),
    Scenario("solve_lane_levels", "solve", _solve(_lib.KERNEL_LANE, levels=True), trees=PLAIN, applies=_solvable),
    Scenario("solve_wave_levels", "solve", _solve(_lib.KERNEL_WAVE, levels=True), trees=PLAIN, applies=_solvable),
    Scenario("solve_team_levels", "solve", _solve(_lib.KERNEL_TEAM, levels=True), trees=PLAIN, applies=_solvable),
    Scenario("repair_exact", "repair_exact", _repair(), trees=PLAIN, applies=_solvable),
    Scenario("query", "query", _query(), "TKNN_QUERY_FORCE_FALLBACK"),
    Scenario("dbscan", "dbscan", _dbscan()),
    Scenario("dbscan_auto", "dbscan_auto", _dbscan_auto(), applies=lambda t: t["n"] >= 17),  # (fewer points than that stay noise for ever)
    Scenario("dbscan_noise", "dbscan_noise", _dbscan_noise()),
    Scenario("dbscan_assign", "dbscan_assign", _dbscan_assign()),
    Scenario("dbscan_query", "dbscan_query", _dbscan_query()),
    Scenario("radius_query_sorted", "radius_query", _radius_query(True), "TKNN_RADIUS_FORCE_FALLBACK"),
    Scenario("radius_query_unsorted", "radius_query", _radius_query(False), "TKNN_RADIUS_FORCE_FALLBACK"),
    Scenario("radius_knn", "radius_knn", _radius_knn(), RKNN),
    Scenario("knn", "knn", _knn(False), "TKNN_KNN_FORCE_FALLBACK"),
    Scenario("knn_own", "knn", _knn(True), "TKNN_KNN_FORCE_FALLBACK"),
    Scenario("periodic_knn", "periodic_knn", _periodic_knn(), "TKNN_PERIODIC_KNN_FORCE_FALLBACK"),
    Scenario("batch_knn", "batch_knn", _batch_knn(), "TKNN_BATCH_KNN_FORCE_FALLBACK", trees=("n1025b3",), applies=lambda t: t["batch"] is not None),
    Scenario("emst", "emst", _emst(False)),
    Scenario("emst_mutual", "emst", _emst(True), applies=lambda t: t["n"] > MIN_SAMPLES),
    Scenario("linkage", "linkage", _linkage(0), trees=PLAIN, bare=True),
    Scenario("linkage_host_finish", "linkage", _linkage(1), trees=PLAIN, bare=True),
    Scenario("hdbscan_labels", "hdbscan_labels", _hdbscan_labels(), trees=PLAIN, bare=True),
    Scenario("hdbscan", "hdbscan", _hdbscan()),
    Scenario("fps", "fps", _fps(), trees=("n1025", "n17ids", "nan700", "n1025b3")),
    Scenario("radius_nms", "radius_nms", _nms(False), "TKNN_NMS_FORCE_FALLBACK", trees=("n1025", "n17ids", "nan700", "n1025b3")),
    Scenario("radius_nms_scored", "radius_nms", _nms(True), "TKNN_NMS_FORCE_FALLBACK"),
    Scenario("radius_nms_apart", "radius_nms", _nms(False, apart=True), "TKNN_NMS_FORCE_FALLBACK", trees=("nan700", "n17ids")),
    Scenario("radius_reduce_count", "radius_reduce", _reduce("one", 0, True), "TKNN_REDUCE_FORCE_FALLBACK", trees=("n1025", "n17ids", "nan700", "n1025b3")),
    Scenario("radius_reduce_gauss5", "radius_reduce", _reduce("gauss", 5, False), "TKNN_REDUCE_FORCE_FALLBACK", trees=("n1025", "n17ids", "nan700", "n1025b3")),
    Scenario("local_pca_radius", "local_pca", _pca((True, None), False), "TKNN_PCA_FORCE_FALLBACK"),
    Scenario("local_pca_k", "local_pca", _pca((None, 16), True), "TKNN_PCA_FORCE_FALLBACK"),
    Scenario("local_pca_both", "local_pca", _pca((True, 16), False), "TKNN_PCA_FORCE_FALLBACK"),
    Scenario("halo_select", "halo_select", _halo_select()),
    Scenario("halo_select_fixed", "halo_select_fixed", _halo_select_fixed()),
    Scenario("halo_phases", "halo_phases", _phases(), trees=PLAIN, applies=lambda t: _solvable(t) and t["batch"] is None),
    Scenario("halo_phases_poisoned_between", "halo_phases", _phases(True), trees=PLAIN, applies=lambda t: _solvable(t) and t["batch"] is None),
)
BY_NAME = {s.name: s for s in TABLE}
assert len(BY_NAME) == len(TABLE)

# ---- what only the guarded-output test reads -------------------------------------------------------------------------------------------
QUERY_COUNTS = (1, 63, 65)  # of n1025's 96 queries: one, one short of a wave, one more than a wave
TAKES_QUERIES = ("query", "dbscan_query", "radius_query_sorted", "radius_query_unsorted", "radius_knn", "knn", "periodic_knn", "batch_knn",
                 "radius_reduce_gauss5", "local_pca_radius", "local_pca_both")


def query_trees(s):
    """The query-count variants the scenario also runs on: those of n1025 (of the batched tree for batch_knn), if it takes queries."""
    if s.name not in TAKES_QUERIES:
        return ()
    return tuple("%sq%d" % ("n1025b3" if s.call == "batch_knn" else "n1025", m) for m in QUERY_COUNTS)


ROW_KS = (1, 16, 17, 64)  # the register lists' capacities and their borders: where a list wider than the row is written out
OWN = ("own",)
MS_FALLBACK, FPFH_FALLBACK, ICP_FALLBACK = "TKNN_MEANSHIFT_FORCE_FALLBACK", "TKNN_FPFH_FORCE_FALLBACK", "TKNN_ICP_FORCE_FALLBACK"


def _at_every_k():
    out = []
    for k in ROW_KS:
        own, asked = dict(trees=("n1025",), k=k), dict(trees=("n1025q65",), k=k)
        out += [Scenario("solve_lane_k%d" % k, "solve", _solve(_lib.KERNEL_LANE, k=k), applies=_solvable, **own),
                Scenario("solve_wave_k%d" % k, "solve", _solve(_lib.KERNEL_WAVE, k=k), applies=_solvable, **own),
                Scenario("solve_team_k%d" % k, "solve", _solve(_lib.KERNEL_TEAM, k=k), applies=_solvable, **own),
                Scenario("query_k%d" % k, "query", _query(k), "TKNN_QUERY_FORCE_FALLBACK", **asked),
                Scenario("radius_knn_k%d" % k, "radius_knn", _radius_knn(k), RKNN, **asked),
                Scenario("knn_k%d" % k, "knn", _knn(False, k), "TKNN_KNN_FORCE_FALLBACK", **asked),
                Scenario("knn_own_k%d" % k, "knn", _knn(True, k), "TKNN_KNN_FORCE_FALLBACK", **own),
                Scenario("periodic_knn_k%d" % k, "periodic_knn", _periodic_knn(k), "TKNN_PERIODIC_KNN_FORCE_FALLBACK", **asked),
                Scenario("batch_knn_k%d" % k, "batch_knn", _batch_knn(k), "TKNN_BATCH_KNN_FORCE_FALLBACK", trees=("n1025b3q65",), k=k),
                Scenario("local_pca_k%d" % k, "local_pca", _pca((None, 16), False, k=k), "TKNN_PCA_FORCE_FALLBACK", **asked)]
    return out


GUARDED_ONLY = tuple(_at_every_k()) + (
    Scenario("batch_layout", "batch_layout", _batch_layout(), trees=("n1025b3",)),
    Scenario("solve_unfinished", "solve", _solve_unfinished(), trees=PLAIN, applies=_solvable),
    Scenario("query_unfinished", "query", _query_unfinished(), "TKNN_QUERY_FORCE_FALLBACK", trees=("n1025", "nan700")),  # (of n17ids no query is served in two rounds)
    Scenario("mean_shift_modes_flat", "mean_shift_modes", _mean_shift_modes("flat"), MS_FALLBACK, trees=OWN, bare=True),
    Scenario("mean_shift_modes_gauss", "mean_shift_modes", _mean_shift_modes("gauss"), MS_FALLBACK, trees=OWN, bare=True),
    Scenario("mean_shift_modes_own", "mean_shift_modes", _mean_shift_modes("flat", own=True), MS_FALLBACK, trees=OWN, bare=True),
    Scenario("mean_shift", "mean_shift", _mean_shift(), MS_FALLBACK, trees=OWN, bare=True),
    Scenario("fpfh", "fpfh", _fpfh(), FPFH_FALLBACK, trees=OWN, bare=True, by_spec=FPFH_BY_SPEC),
    Scenario("icp_point_to_point", "icp", _icp("point_to_point"), ICP_FALLBACK, trees=OWN, bare=True),
    Scenario("icp_point_to_plane", "icp", _icp("point_to_plane"), ICP_FALLBACK, trees=OWN, bare=True),
    Scenario("match_features", "match_features", _global_calls("match."), trees=OWN, bare=True),
    Scenario("ransac", "ransac", _global_calls("ransac."), trees=OWN, bare=True),
)
GUARDED = TABLE + GUARDED_ONLY
GUARDED_BY_NAME = {s.name: s for s in GUARDED}
assert len(GUARDED_BY_NAME) == len(GUARDED)
