"""What TrueKNN.mean_shift_modes (tknnMeanShift, include/owlknn_meanshift.h), TrueKNN.mean_shift and bin_seeds must give, restated in
numpy, the tolerance a step is held to, and the sets the tests share.  No tests here.

One step from x (fp32): the neighbours are the points p of P with the fp32 distance sqrt((dx*dx + dy*dy) + dz*dz) <= r, exactly as
reduce_spec.members finds them (brute force, a NaN on either side is no neighbour, nothing is "self"); d = p - x is the fp32 offset;
the weight w of a neighbour is reduce_spec.weights64's ("flat" is its "one"); W = sum w, a = sum w d, s = a / W, x' = x + s, shift =
|s|, all in float64.  The loop keeps its positions in fp32, as the call does -- x' is rounded after each step, the next predicate is
taken at the rounded position -- and follows the header: NaN seed INVALID; no neighbour EMPTY, x unchanged; a NaN shift INVALID, x
unchanged; shift <= tol CONVERGED; max_iterations steps RUNNING.

The tolerance of one step is derived, not measured, in reduce_spec's manner, u = 2^-24 and c_K its weight constant.  The device sums
len fp32 terms w d per axis and len terms w: by reduce_spec's bound
    dA <= 2 u ((len + 2) sum|w d| + c_K sum|d|)      dW <= 2 u ((len + 2) W + c_K len)
(the product w d is the "w v" of that bound with v = d; d itself is exact input: the walk's own fp32 subtraction, which the spec
repeats).  s = a / W to first order errs by (dA + |s| dW) / W, plus u |s| for the division; x' = x + s adds one rounding, u |x'|:
    |x' - want| <= (dA + |s| dW) / W + u (|s| + |x'|) + 1e-37                                        per axis
    |W - want|  <= dW
    |shift - want| <= |e| + 4 u shift + 1e-37,   e the vector of (dA + |s| dW) / W + u |s| per axis
(shift is a root of three squares and two sums of the computed s: each of the five operations within u relative, the root halves the
relative error of its argument: under 4 u; the error of s moves the norm by at most its own norm).  Counts are compared exactly.
Nothing here depends on where the cloud sits: the offsets are differences.  The recipe that sums w p over absolute coordinates has
sum|w p| where this has sum|w d| -- a cloud at +1000 with r = 0.1 loses four digits (test_meanshift_expectations holds it to that).
"""
import numpy as np

from owlraytracing_amd.datasets import pad_to_3d

import nms_spec
import query_spec as qs
import reduce_spec as rd

U = rd.U
KERNELS = ("flat", "gauss", "epanechnikov")
RUNNING, CONVERGED, EMPTY, INVALID = 0, 1, 2, 3


def weight_name(kernel):
    """reduce_spec's name of a mean-shift kernel."""
    return "one" if kernel == "flat" else kernel


def default_radius(kernel, bandwidth):
    return np.float32(3.0 * float(bandwidth)) if kernel == "gauss" else np.float32(bandwidth)


def step(P, X, r, kernel="flat", h=None):
    """One step from every row of X (fp32): dict(counts (m,) int64, len, wsum (m,) float64, a, absa, absd (m,3) float64 -- the sums
    of w d, |w d| and |d| --, s (m,3), new (m,3) = x + s, shift (m,) float64; rows without neighbours: s, shift NaN, new = x)."""
    P = pad_to_3d(np.asarray(P, np.float32))
    X = np.ascontiguousarray(X, np.float32)
    m = len(X)
    mem = rd.members(P, X, r)
    rowid = np.repeat(np.arange(m), mem["lengths"])
    w = rd.weights64(weight_name(kernel), mem["d2"], mem["d"], r, h)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (P[mem["idx"]] - X[rowid]).astype(np.float32).astype(np.float64)  # the fp32 offsets
    W = np.bincount(rowid, weights=w, minlength=m).astype(np.float64)
    a, absa, absd = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 3))
    for c in range(3):
        a[:, c] = np.bincount(rowid, weights=w * d[:, c], minlength=m)
        absa[:, c] = np.bincount(rowid, weights=np.abs(w * d[:, c]), minlength=m)
        absd[:, c] = np.bincount(rowid, weights=np.abs(d[:, c]), minlength=m)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = a / W[:, None]
    x64 = X.astype(np.float64)
    has = mem["lengths"] > 0
    new = np.where(has[:, None], x64 + s, x64)
    with np.errstate(invalid="ignore"):
        shift = np.sqrt((s * s).sum(axis=1))
    return {"counts": mem["lengths"].copy(), "len": mem["lengths"].copy(), "wsum": W, "a": a, "absa": absa, "absd": absd, "s": s, "new": new,
            "shift": shift}


def tolerances(want, kernel, r, h=None):
    """dict(new (m,3), wsum (m,), shift (m,)) for the rows with neighbours (the module docstring); NaN elsewhere."""
    ck = rd.c_k(weight_name(kernel), r, h)
    ln = want["len"].astype(np.float64)
    dA = 2.0 * U * ((ln[:, None] + 2.0) * want["absa"] + ck * want["absd"])
    dW = 2.0 * U * ((ln + 2.0) * want["wsum"] + ck * ln)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.abs(want["s"])
        e = (dA + s * dW[:, None]) / want["wsum"][:, None] + U * s
        t_new = e + U * np.abs(want["new"]) + 1e-37
        t_shift = np.sqrt((e * e).sum(axis=1)) + 4.0 * U * want["shift"] + 1e-37
    return {"new": t_new, "wsum": dW + 1e-37, "shift": t_shift}


def compare_step(got, want, kernel, r, h=None, X=None):
    """Holds one step of the call (numpy arrays modes, counts, wsum, shift, status, iterations; max_iterations = 1, tol = 0) to the
    spec's step `want` from the seeds X: counts exactly; rows with neighbours inside the tolerance, one step taken; rows without:
    EMPTY (a NaN seed INVALID), the position the seed's bits, count and wsum 0, shift +inf, no step."""
    X = np.ascontiguousarray(X, np.float32)
    tol = tolerances(want, kernel, r, h)
    assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"], want["counts"]), "counts differ"
    has = want["len"] > 0
    nan_seed = np.isnan(X).any(axis=1)
    assert not (has & nan_seed).any()
    for name, g, w in (("modes", got["modes"], want["new"]), ("wsum", got["wsum"], want["wsum"]), ("shift", got["shift"], want["shift"])):
        assert g.dtype == np.float32
        err = np.abs(g.astype(np.float64) - w)[has]
        t = tol["new" if name == "modes" else name][has]
        assert np.isfinite(g[has]).all() and (err <= t).all(), "%s: %g over the bound" % (name, (err - t).max())
    # (tol = 0: only a shift of exactly 0 converges -- a seed alone with itself)
    assert np.array_equal(got["status"][has], np.where(got["shift"][has] == 0, CONVERGED, RUNNING).astype(np.uint8)) and (got["iterations"][has] == 1).all()
    none = ~has
    assert np.array_equal(got["modes"][none].view(np.uint32), X[none].view(np.uint32)), "a seed without neighbours stays where it is, bit for bit"
    assert (got["wsum"][none] == 0).all() and np.isposinf(got["shift"][none]).all() and (got["iterations"][none] == 0).all()
    assert np.array_equal(got["status"][none], np.where(nan_seed[none], INVALID, EMPTY).astype(np.uint8))


def loop(P, seeds, r, kernel="flat", h=None, tol=0.0, max_iterations=300):
    """The header's loop: dict(modes (m,3) float32, counts, wsum, shift, iterations, status, passes, walks).  seeds None: P's rows."""
    P = pad_to_3d(np.asarray(P, np.float32))
    X = (P if seeds is None else np.ascontiguousarray(seeds, np.float32)).copy()
    m = len(X)
    tol = float(np.float32(tol))
    counts, wsum = np.zeros(m, np.int64), np.zeros(m)
    shift, iters = np.full(m, np.inf), np.zeros(m, np.int64)
    status = np.full(m, RUNNING, np.uint8)
    active = np.arange(m)
    passes = walks = 0
    while len(active) and passes < max_iterations:
        st = step(P, X[active], r, kernel, h)
        passes += 1
        walks += len(active)
        keep = np.zeros(len(active), bool)
        for t, j in enumerate(active):
            counts[j], wsum[j] = st["counts"][t], st["wsum"][t]
            if np.isnan(X[j]).any():
                status[j] = INVALID
            elif st["counts"][t] == 0:
                status[j] = EMPTY
            elif np.isnan(st["shift"][t]):
                status[j], shift[j] = INVALID, np.nan
            else:
                X[j] = st["new"][t].astype(np.float32)
                shift[j] = st["shift"][t]
                iters[j] += 1
                if np.float32(shift[j]) <= tol:
                    status[j] = CONVERGED
                else:
                    keep[t] = iters[j] < max_iterations
        active = active[keep]
    return {"modes": X, "counts": counts, "wsum": wsum, "shift": shift, "iterations": iters, "status": status, "passes": passes, "walks": walks}


def merge_and_label(P, modes, scores, status, counts, bandwidth, merge_radius=None, cluster_all=True, min_count=1):
    """TrueKNN.mean_shift's second half: dict(centers (c,3) float32, scores (c,) float32, labels (n,) int64, candidates (rows of the
    seeds)).  Candidates: CONVERGED with counts >= min_count; the greedy merge is radius_nms's (nms_spec.brute: the larger score
    stays, the smaller row among equals); centres by descending score, then ascending candidate row; a point's label is its nearest
    centre in the fp32 distance, the smaller index among equals -- with cluster_all False only within `bandwidth` --, -1 for a NaN."""
    P = pad_to_3d(np.asarray(P, np.float32))
    cand = np.nonzero((np.asarray(status) == CONVERGED) & (np.asarray(counts) >= min_count))[0]
    labels = np.full(len(P), -1, np.int64)
    if len(cand) == 0:
        return {"centers": np.zeros((0, 3), np.float32), "scores": np.zeros(0, np.float32), "labels": labels, "candidates": cand}
    M = np.ascontiguousarray(np.asarray(modes, np.float32)[cand])
    sc = np.asarray(scores)[cand].astype(np.float32)
    keep = nms_spec.brute(M, np.float32(bandwidth if merge_radius is None else merge_radius), scores=sc)["keep"]
    rows = np.nonzero(keep)[0]
    rows = rows[np.argsort(-sc[rows].astype(np.float64), kind="stable")]
    centers = M[rows]
    for s0 in range(0, len(P), 4096):
        with np.errstate(invalid="ignore", over="ignore"):
            d = qs.distance32(centers[None, :, :], P[s0:s0 + 4096, None, :])
        ok = np.isfinite(d) if cluster_all else (d <= np.float32(bandwidth))
        d = np.where(ok, d, np.inf)
        labels[s0:s0 + 4096] = np.where(ok.any(axis=1), np.argmin(d, axis=1), -1)
    return {"centers": centers, "scores": sc[rows], "labels": labels, "candidates": cand}


def bin_seeds(P, bin_size, min_bin_freq=1):
    """sklearn's get_bin_seeds in fp32: the bins round(p / bin_size) (half to even) that hold >= min_bin_freq points, times bin_size,
    in ascending (x, y, z) bin order; rows of P with a coordinate that is not finite are left out."""
    P = pad_to_3d(np.asarray(P, np.float32))
    P = P[np.isfinite(P).all(axis=1)]
    if len(P) == 0:
        return np.zeros((0, 3), np.float32)
    bins = np.round(P / np.float32(bin_size)).astype(np.int64)
    uniq, freq = np.unique(bins, axis=0, return_counts=True)  # lexicographic
    return (uniq[freq >= min_bin_freq].astype(np.float32) * np.float32(bin_size)).astype(np.float32)


def same_partition(a, b):
    """Whether two label arrays name the same partition (labels up to renaming; -1 stays -1)."""
    a, b = np.asarray(a), np.asarray(b)
    if len(a) != len(b) or not np.array_equal(a == -1, b == -1):
        return False
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


# ---- the sets ----------------------------------------------------------------------------------------------------------------------------
BLOB_CENTRES = np.float32([[0.2, 0.2, 0.2], [0.8, 0.2, 0.3], [0.3, 0.8, 0.7], [0.8, 0.8, 0.8]])
BLOB_SIGMA = 0.02
BLOB_KERNELS = {"flat": dict(bandwidth=0.08, radius=0.08), "gauss": dict(bandwidth=0.03, radius=0.09)}
_cache = {}


def blobs():
    """(P (4000,3) float32, component (4000,) int64): four Gauss blobs, seed 12."""
    if "blobs" not in _cache:
        rng = np.random.default_rng(12)
        n = 4000
        comp = rng.integers(0, 4, n)
        P = (BLOB_CENTRES[comp].astype(np.float64) + BLOB_SIGMA * rng.standard_normal((n, 3))).astype(np.float32)
        P.setflags(write=False)
        comp.setflags(write=False)
        _cache["blobs"] = (P, comp)
    return _cache["blobs"]


def blob_means():
    P, comp = blobs()
    return np.stack([P[comp == c].astype(np.float64).mean(axis=0) for c in range(4)])


def blob_loop(kernel):
    """loop(..) over the blobs' own points with BLOB_KERNELS[kernel], tol = 1e-3 bandwidth, at most 10 passes; made once."""
    if ("blob_loop", kernel) not in _cache:
        bw, r = BLOB_KERNELS[kernel]["bandwidth"], np.float32(BLOB_KERNELS[kernel]["radius"])
        _cache[("blob_loop", kernel)] = loop(blobs()[0], None, r, kernel, np.float32(bw), tol=1e-3 * bw, max_iterations=10)
    return _cache[("blob_loop", kernel)]


def uniform_case():
    """(P (5000,3), seeds (3000,3)) uniform in the unit cube: about 10 neighbours within 0.08."""
    if "uniform" not in _cache:
        P = np.random.default_rng(31).random((5000, 3), dtype=np.float32)
        X = np.random.default_rng(32).random((3000, 3), dtype=np.float32)
        P.setflags(write=False)
        X.setflags(write=False)
        _cache["uniform"] = (P, X)
    return _cache["uniform"]


def want_step(key, P, X, r, kernel, h):
    """step(..) made once per key and shared (do not write to it)."""
    key = ("step", key, kernel, float(r))
    if key not in _cache:
        _cache[key] = step(P, X, r, kernel, h)
    return _cache[key]
