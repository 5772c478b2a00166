"""What TrueKNN.fpfh (tknnFpfh, include/owlknn_fpfh.h) must give, restated in numpy, the bounds its histograms are held to, and the
cases its tests share.  No tests here.

Neighbour sets.  N_i is radius_query's row of point i less the row i itself (reduce_spec.members with skip_self: the literal fp32
predicate sqrt((dx*dx + dy*dy) + dz*dz) <= r by brute force; a coinciding duplicate stays in, a NaN point is nobody's neighbour).
The offsets dp = p_j - p_i and the squared distances d2 are the fp32 values the call itself has, bit for bit; so the rules
"d2 == 0" and "1 / d2 finite" are decided exactly.

Features.  From the fp32 normals and offsets, every operation in float64, by the header's seven steps.  A pair is DEGENERATE (enters
no histogram, counts into skipped_pairs) if d2 == 0, vn == 0, a component of either normal is not finite or a feature is not finite.

Margins.  The fp32 evaluation (csrc/fpfh_pair.h) differs from the float64 one by roundings, u = 2^-24 each, times the conditioning
of each step.  To first order, with L = |dp|, N1 = |n1|, N2 = |n2| (lengths about 1), per pair:
  a_k = (n . dp) / f4      three products and two additions on offsets that carry one rounding: 4 u N L; d2 carries 5 u, its root
                           3.5 u, the quotient one more: |da| <= 4 u N + 4.5 u |a| <= 8.5 u N.  f3 is +-a: ABSOLUTE, 8.5 u N.
  v = dp x n1              each component a difference of two products: 3 u (|ab| + |cd|), over the vector <= 4.25 u L N1.  The unit
                           vector v / vn moves by that over vn, kappa = L N1 / vn >= 1 times 4.25 u, plus vn's own 3.5 u and the
                           quotient's: |dv| <= (4.25 kappa + 4.5) u <= 8.75 kappa u.
  f2 = v . n2              |df2| <= (8.75 kappa + 3) u N2 <= 11.75 kappa u N2: grows with f4 / vn.
  f1 = atan2(w . n2, n1 . n2), w = n1 x v:  |dw| <= 13 kappa u N1, the numerator moves by <= 16 kappa u N1 N2, the denominator by
                           3 u N1 N2, and an angle moves by the move of its point over its distance h = hypot(w . n2, n1 . n2) from
                           the origin: (19 kappa N1 N2 / h) u, plus atan2f's own 3 ulps at pi, 12 u: grows with kappa and with 1 / h.
The bins are taken of the scaled values t1 = 11 (f1 + pi) / (2 pi), t2 = 11 (f2 + 1) / 2, t3 = 11 (f3 + 1) / 2: the feature's error
times 11 / (2 pi) = 1.75 or 5.5, plus the scaling's own roundings (22 u for f2 and f3; 33 u and the 8 u of fp32 pi for f1):
    t3: (46.75 N + 22) u      t2: (64.6 kappa N2 + 22) u      t1: (33.25 kappa N1 N2 / h + 62) u
Each is below MARGIN_C = 96 times u times its conditioning max(1, N), kappa max(1, N2), kappa max(1, N1 N2 / h): the margin used.
The role swap compares |a1| with |a2|: it can flip where ||a1| - |a2|| <= 17 u N <= margin3 / 5.5.

Uncertain pairs.  A (pair, feature) is UNCERTAIN if its scaled value lies within its margin of an interior bin edge 1 .. 10; for f1
also of 0 or 11 (+-pi: the wrap sends bin 10 to bin 0); or if the swap can flip and the other assignment of the roles gives another
bin or is itself uncertain (a plane with equal normals has a1 = a2 = 0 on every pair, and the same three features either way: not
uncertain).  A pair whose vn is so small that a margin reaches a whole bin is uncertain by the first rule, whether it enters or not.
A pair with d2 < 2^-100 is uncertain in all three features: its squares are subnormal or close to it and carry fewer bits than u
promises, so the margins do not hold for it (whether it enters the blend, 1 / d2 being finite or not, is decided exactly all the same).
The bound on counts: per row and feature, the sum over the 11 bins of |c_gpu - c_spec| <= 2 U, U the row's uncertain pairs of that
feature (a pair that moves changes two bins by one; a pair that enters on one side only, one).

SPFH and FPFH.  The spec is FED the counts under test and computes in float64.  Every term is non-negative, so every bound is
relative to the value itself, gamma(k) = k u / (1 - k u):
  SPFH = c * (100 / valid): the quotient and the product, k = 2 (the count is exact below 2^24).
  A = sum of SPFH_j * (1 / d2): a term carries SPFH's 2, the reciprocal's and the product's: 4; a sum of len terms in any order
  len - 1 more: len + 3.  S adds 11 of them: len + 13.  A * (100 / S): (len + 3) + (len + 13) + 2 = 2 len + 18.  Plus SPFH (2) in
  one more addition: k = 2 len + 20 covers it, len the row's length.  Without the self term the same bound holds.
"""
import numpy as np

from owlraytracing_amd.datasets import pad_to_3d

import reduce_spec as rsd

U = 2.0 ** -24
MARGIN_C = 96.0
BINS = 11
UNCERTAIN_CAP = 0.01
TINY_D2 = np.float32(2.0 ** -100)


def members(P, r):
    """The rows N_i in CSR form (reduce_spec.members, own points, the row itself left out)."""
    return rsd.members(P, None, r, skip_self=True)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _oriented(n1, n2, dp, L, f3):
    """The features of the pairs with the roles given: dict(t (3, p) scaled values, m (3, p) margins, ok (p,): vn > 0 and finite)."""
    with np.errstate(all="ignore"):
        v = np.cross(dp, n1)
        vn = np.sqrt(_dot(v, v))
        vh = v / vn[:, None]
        w = np.cross(n1, vh)
        f2 = _dot(vh, n2)
        y, x = _dot(w, n2), _dot(n1, n2)
        f1 = np.arctan2(y, x)
        N1, N2 = np.sqrt(_dot(n1, n1)), np.sqrt(_dot(n2, n2))
        kappa = L * N1 / vn
        h = np.hypot(y, x)
        m3 = MARGIN_C * U * np.maximum(1.0, np.maximum(N1, N2))
        m2 = MARGIN_C * U * kappa * np.maximum(1.0, N2)
        m1 = MARGIN_C * U * kappa * np.maximum(1.0, N1 * N2 / h)
        t = np.stack([BINS * (f1 + np.pi) / (2 * np.pi), BINS * (f2 + 1.0) * 0.5, BINS * (f3 + 1.0) * 0.5])
        m = np.stack([m1, m2, m3])
        m[np.isnan(m)] = np.inf
        ok = (vn > 0) & np.isfinite(f1) & np.isfinite(f2) & np.isfinite(f3)
    return {"t": t, "m": m, "ok": ok}


def _bins(t):
    with np.errstate(invalid="ignore"):
        return np.clip(np.floor(np.where(np.isfinite(t), t, 0.0)), 0, BINS - 1).astype(np.int64)


def _near_edge(t, m):
    """(3, p) bool: the scaled value is within its margin of an edge that changes the bin."""
    with np.errstate(invalid="ignore"):
        k = np.clip(np.rint(t), 1, BINS - 1)  # the nearest interior edge
        near = np.abs(t - k) <= m
        near[0] |= (t[0] <= m[0]) | (t[0] >= BINS - m[0])  # the wrap at +-pi
        near |= ~np.isfinite(t) | ~np.isfinite(m)
    return near


def pair_features(P, normals, mem, chunk=400000):
    """Per pair of the rows `mem` (in their order): dict(src (p,) the row, enters (p,) bool, bins (3, p), uncertain (3, p) bool)."""
    P = pad_to_3d(np.asarray(P, np.float32))
    normals = np.asarray(normals, np.float32)
    src_all = np.repeat(np.arange(len(mem["lengths"])), mem["lengths"])
    total = len(src_all)
    enters, bins, unc = np.zeros(total, bool), np.zeros((3, total), np.int64), np.zeros((3, total), bool)
    for s in range(0, total, chunk):
        src, dst = src_all[s:s + chunk], mem["idx"][s:s + chunk]
        with np.errstate(all="ignore"):
            dp = (P[dst] - P[src]).astype(np.float64)  # the fp32 offsets, as the call has them
            ni, nj = normals[src].astype(np.float64), normals[dst].astype(np.float64)
            d2_32 = mem["d2"][s:s + chunk]
            finite = np.isfinite(ni).all(axis=1) & np.isfinite(nj).all(axis=1)
            L = np.sqrt(_dot(dp, dp))
            a1, a2 = _dot(ni, dp) / L, _dot(nj, dp) / L
            swap = np.abs(a1) < np.abs(a2)
            sw = swap[:, None]
            first = _oriented(np.where(sw, nj, ni), np.where(sw, ni, nj), np.where(sw, -dp, dp), L, np.where(swap, -a2, a1))
            other = _oriented(np.where(sw, ni, nj), np.where(sw, nj, ni), np.where(sw, dp, -dp), L, np.where(swap, a1, -a2))
            ok = (d2_32 > 0) & finite & first["ok"]
            b, bo = _bins(first["t"]), _bins(other["t"])
            u = _near_edge(first["t"], first["m"])
            can_flip = np.abs(np.abs(a1) - np.abs(a2)) <= first["m"][2] / 5.5
            u |= can_flip[None, :] & (_near_edge(other["t"], other["m"]) | (bo != b) | ~other["ok"][None, :])
            u |= (d2_32 < TINY_D2)[None, :]
            u &= ((d2_32 > 0) & finite)[None, :]  # (these two rules are exact: such a pair is skipped on both sides)
        enters[s:s + chunk], bins[:, s:s + chunk], unc[:, s:s + chunk] = ok, b, u
    return {"src": src_all, "enters": enters, "bins": bins, "uncertain": unc}


def histograms(feat, n):
    """dict(counts (n, 33) int64, uncertain (n, 3) int64: U per row and feature, skipped: the degenerate pairs, pairs)."""
    counts, unc = np.zeros((n, 3 * BINS), np.int64), np.zeros((n, 3), np.int64)
    e = feat["enters"]
    for f in range(3):
        np.add.at(counts, (feat["src"][e], f * BINS + feat["bins"][f][e]), 1)
        unc[:, f] = np.bincount(feat["src"][feat["uncertain"][f]], minlength=n)
    return {"counts": counts, "uncertain": unc, "skipped": int((~e).sum()), "pairs": len(e)}


def spfh64(counts):
    """SPFH in float64 from integer counts (n, 33)."""
    c = np.asarray(counts).astype(np.float64)
    valid = c[:, :BINS].sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(valid[:, None] > 0, c * (100.0 / valid)[:, None], 0.0)


def fpfh64(counts, mem, self_term=True):
    """FPFH in float64 from the counts (n, 33) and the rows: the weights from the fp32 d2, entering as the header says."""
    n = len(mem["lengths"])
    S = spfh64(counts)
    src = np.repeat(np.arange(n), mem["lengths"])
    d2 = mem["d2"]
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        w32 = np.float32(1) / d2
    ent = (d2 > 0) & np.isfinite(w32)
    w = 1.0 / d2[ent].astype(np.float64)
    A = np.zeros((n, 3 * BINS))
    for b in range(3 * BINS):
        A[:, b] = np.bincount(src[ent], weights=S[mem["idx"][ent], b] * w, minlength=n)
    out = np.zeros_like(A)
    for f in range(3):
        cols = slice(f * BINS, (f + 1) * BINS)
        tot = A[:, cols].sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, cols] = np.where(tot[:, None] > 0, A[:, cols] * (100.0 / tot)[:, None], 0.0)
    return out + S if self_term else out


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def check_counts(got, hist):
    """The 2 U bound, per row and feature."""
    got = np.asarray(got).astype(np.int64)
    assert got.shape == hist["counts"].shape and (got >= 0).all()
    for f in range(3):
        cols = slice(f * BINS, (f + 1) * BINS)
        diff = np.abs(got[:, cols] - hist["counts"][:, cols]).sum(axis=1)
        bad = np.nonzero(diff > 2 * hist["uncertain"][:, f])[0]
        assert len(bad) == 0, "feature %d: %d rows beyond 2 U (row %d: off by %d with U = %d)" % (f + 1, len(bad), bad[0], diff[bad[0]], hist["uncertain"][bad[0], f])
    assert np.array_equal(got[:, :BINS].sum(axis=1), got[:, BINS:2 * BINS].sum(axis=1)) and np.array_equal(got[:, :BINS].sum(axis=1), got[:, 2 * BINS:].sum(axis=1))


def check_floats(got, counts, mem, self_term=True, spfh=None, slack=1.0):
    """fpfh (and spfh) against the float64 values made from the counts under test; `slack` times the bound."""
    lens = mem["lengths"].astype(np.float64)[:, None]
    if spfh is not None:
        want = spfh64(counts)
        err = np.abs(np.asarray(spfh, np.float64) - want)
        print("spfh: largest error / bound %.3g" % float((err / np.maximum(gamma(2) * want, 1e-300))[want > 0].max(initial=0)))
        assert spfh.dtype == np.float32 and (err <= slack * gamma(2) * want).all(), "spfh beyond its bound"
    want = fpfh64(counts, mem, self_term)
    err = np.abs(np.asarray(got, np.float64) - want)
    tol = slack * gamma(2 * lens + 20) * want
    print("fpfh: largest error / bound %.3g" % float((err / np.maximum(tol, 1e-300))[want > 0].max(initial=0)))
    assert got.dtype == np.float32 and (err <= tol).all(), "fpfh: %g beyond its bound at %s" % ((err - tol).max(), np.unravel_index(np.argmax(err - tol), err.shape))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def sphere(n, seed):
    """A noisy unit sphere; the normals the radial directions, turned a little at random (no pair is symmetric by construction)."""
    rng = np.random.default_rng(seed)
    d = _unit(rng.standard_normal((n, 3)))
    P = (d * (1.0 + 0.01 * rng.standard_normal((n, 1)))).astype(np.float32)
    return P, _unit(d + 0.05 * rng.standard_normal((n, 3)))


def cube(n, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3), dtype=np.float32), _unit(rng.standard_normal((n, 3)))


def plane(n, seed):
    rng = np.random.default_rng(seed)
    P = np.zeros((n, 3), np.float32)
    P[:, :2] = rng.random((n, 2), dtype=np.float32)
    N = np.zeros((n, 3), np.float32)
    N[:, 2] = 1
    return P, N


def _make(name):
    ids = batch = None
    if name == "n1":
        P, N, r = np.float32([[0.25, 0.5, 0.75]]), np.float32([[0, 0, 1]]), 0.5
    elif name == "n17":  # no box pyramid: the lane kernel
        (P, N), r = cube(17, 1), 0.6
    elif name in ("sphere1025", "sphere4200"):
        n = int(name[6:])
        (P, N), r = sphere(n, n), {1025: 0.3, 4200: 0.15}[n]
    elif name in ("cube1025", "cube4200"):
        n = int(name[4:])
        (P, N), r = cube(n, n + 1), {1025: 0.18, 4200: 0.1124}[n]
    elif name in ("plane1025", "plane4200"):
        n = int(name[5:])
        (P, N), r = plane(n, n + 2), {1025: 0.088, 4200: 0.0435}[n]
    elif name == "third":  # about a third of the cloud within r: long rows of leaf blocks (no 1024-point box lies inside such a sphere)
        (P, N), r = cube(4200, 7), 0.45
    elif name == "all1100":  # twice the extent: the box of the first 1024 sorted slots lies inside every sphere and is STREAMED through the
        (P, N), r = cube(1100, 14), 3.5  # team's range list, the other 76 points come by leaf blocks; every row is the whole set
    elif name == "dirty":  # 5 % coinciding duplicates, NaN points, normals that are zero or not finite
        (P, N), r = cube(1200, 8), 0.17
        rng = np.random.default_rng(9)
        P[rng.choice(1200, 60, replace=False)] = P[rng.choice(1200, 60, replace=False)]
        P[[11, 500, 1199], [0, 1, 2]] = np.nan
        N[[3, 700]] = 0
        N[40, 1], N[900, 0], N[901, 2] = np.nan, np.inf, -np.inf
        # two points 1e-20 apart: d2 is positive and subnormal, 1 / d2 overflows: the pair is binned and does not enter the blend
        # (equal normals across the offset: its three features are 0 however few bits the squares carry)
        P[20], P[21] = [0, 0, 0], [1e-20, 0, 0]
        N[20] = N[21] = [0, 0, 1]
    elif name == "ids":  # ids that are a permutation of the rows: everything goes by row all the same
        (P, N), r = cube(800, 10), 0.2
        ids = np.roll(np.random.default_rng(11).permutation(800), 1).astype(np.int32)
    elif name == "batched":  # three clouds in one tree: the labels are ignored
        (P, N), r = sphere(900, 12), 0.32
        batch = np.random.default_rng(13).integers(0, 3, 900).astype(np.int32)
    else:
        raise KeyError(name)
    return {"P": np.ascontiguousarray(P, np.float32), "N": np.ascontiguousarray(N, np.float32), "r": np.float32(r), "ids": ids, "batch": batch,
            "num_batches": None if batch is None else 3}


CASE_NAMES = ("n1", "n17", "sphere1025", "cube1025", "plane1025", "sphere4200", "cube4200", "plane4200", "third", "all1100", "dirty", "ids", "batched")
_cache = {}


def case(name):
    """A named case with its rows and histograms: dict(P, N, r, ids, batch, num_batches, mem, feat, hist), made once and shared
    (do not write to it)."""
    if name not in _cache:
        c = _make(name)
        c["mem"] = members(c["P"], c["r"])
        c["feat"] = pair_features(c["P"], c["N"], c["mem"])
        c["hist"] = histograms(c["feat"], len(c["P"]))
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = c
    return _cache[name]
