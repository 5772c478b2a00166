"""What TrueKNN.radius_reduce (tknnRadiusReduce, include/owlknn_reduce.h) must give, restated in numpy, the tolerance its sums are
held to, and the cases its tests share.  No tests here.

Row j sums over the points p of the built set P with dist(p, q_j) <= r, dist the fp32 formula sqrt((dx*dx + dy*dy) + dz*dz)
(query_spec.distance32), exactly as radius_spec.radius_rows finds them:
  * distance exactly r is inside; nothing is "self" -- with the set's own points as queries (Q None) and skip_self the query's own
    ROW is left out, a coinciding duplicate stays in;
  * a NaN coordinate on either side: not a neighbour.  Batch labels and ids play no part: values go by the caller's row;
  * the weight of a neighbour is computed in float64 from the fp32 squared distance d2, its fp32 root d and the fp32 constants
    the header defines (c = fl(-0.5 / h^2), fl(1 / r^2), fl(2 / r)), with the header's clamps; every sum is in float64.
Brute force: every pair's distance is computed, so the spec cannot share a mistake with a traversal.

The tolerance is derived, not measured.  With u = 2^-24: an fp32 sum of len terms t in any order errs by at most (len - 1) u sum|t|
to first order; a product w * v adds one rounding, u |w v|; every weight is <= 1 and carries an absolute error of at most c_K u
-- c_K = 0 for "one", 16 for the two polynomial weights (at most 8 roundings of quantities <= 2), 2 (x_max + 2) for "gauss" with
x_max = r^2 / (2 h^2) (the argument's rounding, and an exp within one ulp).  With A = sum|w v_c| and V = sum|v_c| over the row:
    |got - want| <= 2 u ((len + 2) A + c_K V) + 1e-37
the factor 2 for the second-order terms and any contraction the compiler picks; wsum: the same with v = 1.  A normalised output
S / W: the two bounds propagated to first order, tol_S / W + |S| tol_W / W^2, plus one rounding of the quotient; rows with
W < 1e-3 len (weights dying at the rim) are left out of that comparison, at most 1 % of a case's rows (the CPU test holds the
cases to it).  Counts are compared exactly.
"""
import numpy as np

from owlraytracing_amd import datasets
from owlraytracing_amd.datasets import pad_to_3d

import query_spec as qs
import radius_spec as rs
import tile_sets

U = 2.0 ** -24
WEIGHTS = ("one", "gauss", "epanechnikov", "cubic_spline")
MAX_CHANNELS = 16
CHANNEL_COUNTS = (0, 1, 3, 4, 5, 8, 16)  # the edges of the tiers 0, <= 4, <= 8, <= 16
RIM_SHARE = 1e-3  # rows with W < RIM_SHARE * len are left out of the normalised comparison
RIM_CAP = 0.01    # ... at most this share of a case's rows


def members(P, Q, r, skip_self=False):
    """The rows in CSR form: dict(offsets (m+1,) int64, idx (total,) int64 rows of P ascending inside a row, d2 (total,) float32,
    d (total,) float32, lengths (m,) int64).  Q None: the rows of P are the queries."""
    P = pad_to_3d(np.asarray(P, np.float32))
    own = Q is None
    Qa = P if own else pad_to_3d(np.asarray(Q, np.float32))
    assert own or not skip_self
    m, r = len(Qa), np.float32(r)
    block = max(1, min(256, 4000000 // max(len(P), 1)))
    lengths = np.zeros(m, np.int64)
    idx, d2s = [], []
    for s in range(0, m, block):
        with np.errstate(invalid="ignore", over="ignore"):
            diff = P[None, :, :] - Qa[s:s + block, None, :]
            x, y, z = diff[..., 0], diff[..., 1], diff[..., 2]
            d2 = ((x * x) + (y * y)) + (z * z)
            near = np.sqrt(d2, dtype=np.float32) <= r  # (NaN <= r is False)
        if skip_self:
            near[np.arange(near.shape[0]), np.arange(s, s + near.shape[0])] = False
        jj, cc = np.nonzero(near)  # row-major: ascending c inside a row
        lengths[s:s + near.shape[0]] = np.bincount(jj, minlength=near.shape[0])
        idx.append(cc.astype(np.int64))
        d2s.append(d2[jj, cc].astype(np.float32))
    d2 = np.concatenate(d2s) if d2s else np.zeros(0, np.float32)
    out = {"offsets": np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), "idx": np.concatenate(idx) if idx else np.zeros(0, np.int64),
           "d2": d2, "d": np.sqrt(d2, dtype=np.float32), "lengths": lengths}
    for a in out.values():
        a.setflags(write=False)
    return out


def constants(weight, r, h=None):
    """The fp32 constant the header defines for the weight (None for "one")."""
    r = float(np.float32(r))
    if weight == "gauss":
        h = float(np.float32(h))
        return np.float32(-0.5 / (h * h))
    if weight == "epanechnikov":
        return np.float32(1.0 / (r * r))
    if weight == "cubic_spline":
        return np.float32(2.0 / r)
    return None


def weights64(weight, d2, d, r, h=None):
    """float64 weights of neighbours with the fp32 squared distances d2 and roots d."""
    d2, d = np.asarray(d2, np.float32).astype(np.float64), np.asarray(d, np.float32).astype(np.float64)
    if weight == "one":
        return np.ones_like(d2)
    k = float(constants(weight, r, h))
    if weight == "gauss":
        return np.exp(d2 * k)
    if weight == "epanechnikov":
        return np.maximum(0.0, 1.0 - d2 * k)
    assert weight == "cubic_spline"
    s = d * k
    return np.where(s <= 1.0, 1.0 - 1.5 * s * s + 0.75 * s * s * s, np.maximum(0.0, 0.25 * (2.0 - s) ** 3))


def c_k(weight, r, h=None):
    """The absolute error of an fp32 weight, in units of u."""
    if weight == "one":
        return 0.0
    if weight == "gauss":
        r, h = float(np.float32(r)), float(np.float32(h))
        return 2.0 * (r * r / (2.0 * h * h) + 2.0)
    return 16.0


def sums(mem, values, weight, r, h=None):
    """dict(counts (m,) int64, wsum (m,) float64, out, A, V (m, C) float64 -- the sums of w v_c, |w v_c| and |v_c| over the row --,
    len (m,), w (total,) float64) of the rows `mem` with the values (n, C) (None: C = 0)."""
    m = len(mem["lengths"])
    rowid = np.repeat(np.arange(m), mem["lengths"])
    w = weights64(weight, mem["d2"], mem["d"], r, h)
    out = {"counts": mem["lengths"].copy(), "len": mem["lengths"].copy(), "w": w, "wsum": np.bincount(rowid, weights=w, minlength=m).astype(np.float64)}
    C = 0 if values is None else values.shape[1]
    S, A, V = np.zeros((m, C)), np.zeros((m, C)), np.zeros((m, C))
    for c in range(C):
        v = np.asarray(values[:, c], np.float32).astype(np.float64)[mem["idx"]]
        with np.errstate(invalid="ignore"):
            S[:, c] = np.bincount(rowid, weights=w * v, minlength=m)
            A[:, c] = np.bincount(rowid, weights=np.abs(w * v), minlength=m)
            V[:, c] = np.bincount(rowid, weights=np.abs(v), minlength=m)
    out.update(out=S, A=A, V=V)
    return out


def bound(length, A, V, ck):
    """The tolerance of one fp32 sum (module docstring); `length` broadcasts against A."""
    return 2.0 * U * ((length + 2.0) * A + ck * V) + 1e-37


def tolerances(want, weight, r, h=None):
    """dict(out (m, C), wsum (m,), norm (m, C), norm_rows (m,) bool: the rows the normalised comparison covers, norm_want (m, C))."""
    ck = c_k(weight, r, h)
    ln = want["len"].astype(np.float64)
    t_out = bound(ln[:, None], want["A"], want["V"], ck)
    t_w = bound(ln, want["wsum"], ln, ck)
    W = want["wsum"]
    rows = (want["len"] > 0) & (W >= RIM_SHARE * ln)
    with np.errstate(divide="ignore", invalid="ignore"):
        Ws = np.where(rows, W, 1.0)[:, None]
        q = want["out"] / Ws
        t_norm = t_out / Ws + np.abs(want["out"]) * t_w[:, None] / (Ws * Ws) + U * np.abs(q) + 1e-37
    return {"out": t_out, "wsum": t_w, "norm": t_norm, "norm_rows": rows, "norm_want": q}


def compare(got, want, weight, r, h=None, normalize=False, channels=None):
    """Holds the arrays of one call (numpy; a missing or None entry was not asked for) to the spec's sums `want`: the counts exactly,
    wsum and out inside the tolerance; with `normalize` out is the quotient, exactly 0 on rows without neighbours, compared on the rows
    the tolerance covers.  `channels`: the call summed the first so many columns of the values `want` was made with."""
    tol = tolerances(want, weight, r, h)
    if got.get("counts") is not None:
        assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"], want["counts"]), "counts differ"
    if got.get("wsum") is not None:
        err = np.abs(got["wsum"].astype(np.float64) - want["wsum"])
        assert got["wsum"].dtype == np.float32 and (err <= tol["wsum"]).all(), "wsum: %g over the bound at row %d" % ((err - tol["wsum"]).max(), int(np.argmax(err - tol["wsum"])))
    if got.get("out") is not None:
        C = got["out"].shape[1] if channels is None else channels
        g = got["out"].astype(np.float64).reshape(len(want["len"]), -1)
        assert g.shape[1] == C
        if not normalize:
            err = np.abs(g - want["out"][:, :C])
            assert (err <= tol["out"][:, :C]).all(), "out: %g over the bound at %s" % ((err - tol["out"][:, :C]).max(), np.unravel_index(np.argmax(err - tol["out"][:, :C]), err.shape))
        else:
            assert (g[want["len"] == 0] == 0).all(), "a row without neighbours normalises to exactly 0"
            rows = tol["norm_rows"]
            err = np.abs(g[rows] - tol["norm_want"][rows, :C])
            assert (err <= tol["norm"][rows, :C]).all(), "normalised out: %g over the bound" % (err - tol["norm"][rows, :C]).max()
            assert np.isfinite(g).all()


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def values_for(n, seed=0):
    """(n, 16) float32 values by row: signed, of mixed magnitude, column 0 positive (masses), columns 1-3 like coordinates."""
    rng = np.random.default_rng(7000 + seed)
    v = rng.standard_normal((n, MAX_CHANNELS)).astype(np.float32)
    v[:, 0] = np.abs(v[:, 0]) + np.float32(0.5)
    v[:, 4:8] *= np.float32(1e3)
    v[:, 12:] *= np.float32(1e-3)
    return v


def _uniform(n, seed, nq, qseed):
    return datasets.uniform3d(n, seed=seed), np.random.default_rng(qseed).random((nq, 3), dtype=np.float32)


def _nearest(P, Q):
    """The smallest positive finite fp32 distance between a query and a point."""
    best = np.inf
    for s in range(0, len(Q), 256):
        with np.errstate(invalid="ignore", over="ignore"):
            d = qs.distance32(P[None, :, :], Q[s:s + 256, None, :])
        ok = np.isfinite(d) & (d > 0)
        if ok.any():
            best = min(best, float(d[ok].min()))
    return np.float32(best)


def _radii(P, Q, mid):
    """The radius classes of a set: `empty` below every positive distance between a query and a point (every row is empty, or holds
    only points that coincide with the query), `mid` (tens of neighbours),
    `half` (about half the set: many boxes inside the sphere, more than a team's range list holds), `all` (twice the extent: everything, the top
    boxes are inside)."""
    clean = P[~np.isnan(P).any(axis=1)]
    lo, hi = clean.min(0).astype(np.float64), clean.max(0).astype(np.float64)
    Qc = Q[~np.isnan(Q).any(axis=1)]
    lo, hi = np.minimum(lo, Qc.min(0)), np.maximum(hi, Qc.max(0))
    extent = float(np.linalg.norm(hi - lo))
    near = _nearest(P, Q)
    out = {"mid": np.float32(mid), "half": np.float32(0.28 * extent), "all": np.float32(2.0 * extent)}
    if np.isfinite(near) and np.nextafter(near, np.float32(0)) > 0:
        out["empty"] = np.float32(np.nextafter(near, np.float32(0)))
    return out


def _make(name):
    ids = batch = None
    own = True
    if name in ("n1", "n15", "n16", "n17"):
        n = int(name[1:])
        P = np.random.default_rng(800 + n).random((n, 3), dtype=np.float32)
        # the queries: jittered copies of the points (every row has a neighbour of weight near 1: no row sits at the rim alone), the
        # first point itself, two far ones that only the largest radius reaches, a NaN
        rng = np.random.default_rng(900 + n)
        near = P[rng.integers(0, n, 100)] + (rng.random((100, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(2e-3)
        Q = np.concatenate([near, P[:1], np.float32([[3, 3, 3], [-2, 0.5, 0.5], [np.nan, 0.5, 0.5]])]).astype(np.float32)
        mid = 0.8
    elif name == "n1025":
        P, Q = _uniform(1025, 41, 96, 42)
        Q[5] = [0.5, np.nan, 0.5]
        mid = 0.2
    elif name == "n66000":
        P, Q = _uniform(66000, 43, 64, 44)
        mid, own = 0.03, False
    elif name in ("duplicates", "planar", "scale_up"):
        P, Q, r0 = qs.make_set(name)
        Q = np.ascontiguousarray(Q[:: max(1, len(Q) // 150)])
        mid, own = {"duplicates": 3, "planar": 15, "scale_up": 5}[name] * r0, False
    elif name == "dup_own":  # a quarter of the points are copies: they stay in a row that skips its own point
        P, Q = tile_sets.with_duplicates(900, 5), np.random.default_rng(46).random((40, 3), dtype=np.float32)
        mid = 0.15
    elif name == "nan":
        P, Q = _uniform(700, 47, 60, 48)
        P[np.random.default_rng(49).choice(700, 45, replace=False), np.random.default_rng(50).integers(0, 3, 45)] = np.nan
        Q[3] = [np.nan, np.nan, np.nan]
        mid = 0.2
    elif name == "ids":  # ids that are a permutation of the rows, none its own row: values go by row all the same
        P, Q = _uniform(800, 51, 60, 52)
        ids = np.roll(np.random.default_rng(53).permutation(800), 1).astype(np.int32)
        ids = np.where(ids == np.arange(800), (ids + 1) % 800, ids).astype(np.int32)
        mid = 0.2
    elif name == "batched":  # three clouds in one tree: the labels are ignored
        P, Q = _uniform(900, 54, 60, 55)
        batch = np.random.default_rng(56).integers(0, 3, 900).astype(np.int32)
        mid = 0.2
    else:
        raise KeyError(name)
    P, Q = np.ascontiguousarray(P, np.float32), np.ascontiguousarray(Q, np.float32)
    return {"P": P, "Q": Q, "ids": ids, "batch": batch, "num_batches": None if batch is None else 3, "own": own, "radii": _radii(P, Q, mid),
            "values": values_for(len(P), seed=len(P))}


SET_NAMES = ("n1", "n15", "n16", "n17", "n1025", "n66000", "duplicates", "planar", "scale_up", "dup_own", "nan", "ids", "batched")
_cache = {}


def case(name):
    """A named set, made once and shared (do not write to it)."""
    if ("case", name) not in _cache:
        c = _make(name)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[("case", name)] = c
    return _cache[("case", name)]


def bandwidth(r):
    """The Gauss bandwidth the tests pair with a radius: the sphere is cut at 2.5 sigma."""
    return np.float32(np.float32(r) / np.float32(2.5))


def rows_of(name, label, mode):
    """The spec's rows of set `name` at its radius `label`; mode: "ext" (the set's queries), "own", "own_skip"."""
    key = ("rows", name, label, mode)
    if key not in _cache:
        c = case(name)
        _cache[key] = members(c["P"], c["Q"] if mode == "ext" else None, c["radii"][label], skip_self=mode == "own_skip")
    return _cache[key]


def want_of(name, label, mode, weight):
    """The spec's sums over rows_of(..) with the set's 16 value columns and bandwidth(r), made once and shared."""
    key = ("want", name, label, mode, weight)
    if key not in _cache:
        c = case(name)
        r = c["radii"][label]
        _cache[key] = sums(rows_of(name, label, mode), c["values"], weight, r, bandwidth(r))
    return _cache[key]


def modes_of(name):
    return ("ext", "own", "own_skip") if case(name)["own"] else ("ext",)


def chunk_case():
    """radius_spec.chunk_case with values: (P, Q, picks, values)."""
    P, Q, picks = rs.chunk_case()
    return P, Q, picks, values_for(len(P), seed=1)


def lattice_case():
    """radius_spec.lattice_case with values: (P, Q, radii, values)."""
    P, Q, radii = rs.lattice_case()
    return P, Q, radii, values_for(len(P), seed=2)
