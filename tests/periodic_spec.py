"""What TrueKNN.periodic_knn (tknnPeriodicKnn, include/owlknn_periodic.h) must return, restated in numpy, and the cases its tests
share.  No tests here.

The cell is lo[3], period[3]; axis a is periodic iff period[a] > 0, 0 means open.  For a point p and a query q, every operation
fp32 and rounded on its own:
    a   = |fl(p_a - q_a)|
    w_a = a                       on an open axis
    w_a = min(a, |fl(L_a - a)|)   on a periodic one
    d2  = (w_x*w_x + w_y*w_y) + w_z*w_z
    d   = sqrt(d2)
A NaN coordinate on either side makes d NaN (np.minimum keeps a NaN).  A value x is IN the cell on a periodic axis iff
x >= lo_a and fl(x - lo_a) <= L_a.
Row j holds the points of P eligible for q_j, ascending in (d, index) -- index = id where ids are given --, cut after k, padded
with idx -1 / dist +inf; counts[j] = min(k, eligible).  Eligible: d finite and d <= r_j (a distance exactly r_j is inside; r_j
must be finite -- FLT_MAX is "none" -- and > 0, else the row is empty); not the point skip[j] names (negative: none); q_j in the
cell on every periodic axis.  Brute force over every pair: no tree, no images, no gate -- every point is looked at once, so none
can appear twice.
"""
import numpy as np

from owlraytracing_amd.datasets import pad_to_3d

K_MAX = 64  # TKNN_MAX_K_REGISTERS
FLT_MAX = np.finfo(np.float32).max
K_ALL = (1, 5, 16, 17, 32, 33, 48, 49, 64)  # every list size of the team kernel and both sides of each boundary

UNIT = (np.float32([0, 0, 0]), np.float32([1, 1, 1]))
CELL = (np.float32([0.1, -0.3, 2.0]), np.float32([0.3, 0.7, 0]))  # non-dyadic, z open


def cell_of(lo, period):
    return np.asarray(lo, np.float32).reshape(3), np.asarray(period, np.float32).reshape(3)


def in_cell(X, lo, period):
    """Per row of X (m,3): in the cell on every periodic axis."""
    lo, period = cell_of(lo, period)
    X = np.asarray(X, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (X >= lo) & ((X - lo) <= period)
    return (ok | ~(period > 0)).all(axis=1)


def wrapped(P, Q, lo, period, wrap=True):
    """(m, n) float32 distances of the formula above; wrap=False: the open distance (every axis taken as open)."""
    lo, period = cell_of(lo, period)
    P, Q = pad_to_3d(np.asarray(P, np.float32)), pad_to_3d(np.asarray(Q, np.float32))
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(P[None, :, :] - Q[:, None, :])
        assert a.dtype == np.float32
        w = [np.minimum(a[..., t], np.abs(period[t] - a[..., t])) if wrap and period[t] > 0 else a[..., t] for t in range(3)]
        d = np.sqrt(((w[0] * w[0]) + (w[1] * w[1])) + (w[2] * w[2]), dtype=np.float32)
    assert d.dtype == np.float32
    return d


def knn_rows(P, Q, k, lo, period, radius=None, radii=None, skip=None, ids=None, block=128):
    """dict(idx (m,k) int32, dist (m,k) float32, counts (m,) int32) of the queries Q against P in the cell."""
    assert radius is None or radii is None
    P, Q = pad_to_3d(np.asarray(P, np.float32)), pad_to_3d(np.asarray(Q, np.float32))
    n, m = len(P), len(Q)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    skip = np.full(m, -1, np.int64) if skip is None else np.asarray(skip, np.int64)
    r = np.full(m, FLT_MAX if radius is None else radius, np.float32) if radii is None else np.asarray(radii, np.float32)
    with np.errstate(invalid="ignore"):
        row_ok = np.isfinite(r) & (r > 0) & in_cell(Q, lo, period)
    idx = np.full((m, k), -1, np.int32)
    dist = np.full((m, k), np.inf, np.float32)
    counts = np.zeros(m, np.int32)
    for s in range(0, m, block):
        d = wrapped(P, Q[s:s + block], lo, period)
        for t in range(d.shape[0]):
            j = s + t
            if not row_ok[j]:
                continue
            with np.errstate(invalid="ignore"):
                c = np.flatnonzero(np.isfinite(d[t]) & (d[t] <= r[j]) & ((ids != skip[j]) | (skip[j] < 0)))
            if len(c) > k:  # (only what lies no farther than the k-th smallest distance can be in the row: less to sort)
                c = c[d[t, c] <= np.partition(d[t, c], k - 1)[k - 1]]
            o = c[np.lexsort((ids[c], d[t, c]))][:k]  # by distance, then by index
            counts[j] = len(o)
            idx[j, :len(o)] = ids[o]
            dist[j, :len(o)] = d[t, o]
    return {"idx": idx, "dist": dist, "counts": counts}


def self_rows(P, k, lo, period, ids=None, **kw):
    """The rows of P's own points: every point left out of its own row, by its id or row (radii: by row)."""
    return knn_rows(P, P, k, lo, period, skip=np.arange(len(P)) if ids is None else ids, ids=ids, **kw)


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
def uniform_in(lo, period, n, seed, open_lo=0.0, open_width=1.0):
    """n uniform points in the cell (clipped into it after rounding); an open axis spans [lo_a + open_lo, .. + open_width]."""
    lo, period = cell_of(lo, period)
    rng = np.random.default_rng(seed)
    u = rng.random((n, 3), dtype=np.float32)
    width = np.where(period > 0, period, np.float32(open_width)).astype(np.float32)
    X = (lo + np.where(period > 0, 0, np.float32(open_lo)).astype(np.float32) + u * width).astype(np.float32)
    for t in range(3):
        if period[t] > 0:  # rounding may carry a value a step outside: take those one step back in
            bad = ~((X[:, t] >= lo[t]) & ((X[:, t] - lo[t]) <= period[t]))
            X[bad, t] = lo[t]
    assert in_cell(X, lo, period).all()
    return np.ascontiguousarray(X)


def uniform_case():
    """(P, Q, lo, period): 2 000 uniform points and 300 queries in the non-dyadic cell, z open over a width of 0.3."""
    lo, period = CELL
    return uniform_in(lo, period, 2000, 81, open_width=0.3), uniform_in(lo, period, 300, 82, open_width=0.3), lo, period


def uniform_ids(n):
    """A permutation plus an offset."""
    return (np.random.default_rng(83).permutation(n) + 1_000_000).astype(np.int32)


LATTICE_K = (1, 3, 6, 7)
LATTICE_SPACING = np.float32(1.0 / 16)


def lattice_case():
    """(P, Q, face): the lattice of spacing 1/16 in the unit cell, all three axes periodic (points at 0, 1/16, .. 15/16: the
    neighbour of x = 0 across the face is x = 15/16); Q: cell centres and edge midpoints next to and across the faces; face: the
    rows of P on the x = 0 face (self-mode rows that cross it)."""
    g = np.arange(16, dtype=np.float32) * LATTICE_SPACING
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(84)
    P = np.ascontiguousarray(P[rng.permutation(len(P))])
    h = LATTICE_SPACING / np.float32(2)
    cells = np.float32([[15, 3, 7], [15, 15, 15], [15, 7, 0], [15, 15, 2], [15, 8, 15], [15, 0, 15]]) * LATTICE_SPACING
    centres = cells + h  # the centre of the last cell of an axis lies at 31/32: the corners at x = 0 are across the face
    edges = cells + np.float32([h, 0, 0])
    Q = np.ascontiguousarray(np.concatenate([centres, edges]).astype(np.float32))
    return P, Q, np.flatnonzero(P[:, 0] == 0)


TINY_N = (1, 2, 16, 17, 65, 20)


def tiny_case(n):
    """(P, Q, ks): n points in the unit cell, k below, at and above n.  The first two points are an anchor and a point next to it,
    and the 12 queries lie around the anchor's antipode (0.4 .. 0.6 away on every axis, wrapped into the cell): every row of at
    least n - 1 entries holds a point farther than half a period, where a walk over shifted images would meet points twice."""
    lo, period = UNIT
    P = uniform_in(lo, period, n, 85 + n)
    anchor = np.float32([0.9, 0.15, 0.55])
    P[0] = anchor
    if n > 1:
        P[1] = anchor + np.float32([0.004, -0.003, 0.002])
    off = np.float32(0.4) + np.random.default_rng(185 + n).random((12, 3), dtype=np.float32) * np.float32(0.2)
    Q = (anchor + off).astype(np.float32)
    Q = np.where(Q >= 1, Q - np.float32(1), Q).astype(np.float32)
    assert in_cell(Q, lo, period).all()
    ks = sorted({1, max(n - 1, 1), min(n, K_MAX), min(n + 1, K_MAX), K_MAX})
    return P, np.ascontiguousarray(Q), ks


def pyramid_case():
    """(P, Q): 70 000 uniform points in the unit cell (a box pyramid of three levels: 4 375 blocks, 69 nodes, 2), 256 queries, half
    of them within 0.01 of a face."""
    lo, period = UNIT
    P = uniform_in(lo, period, 70_000, 86)
    Q = uniform_in(lo, period, 256, 87)
    rng = np.random.default_rng(88)
    near = rng.random(128, dtype=np.float32) * np.float32(0.01)
    axis, side = rng.integers(0, 3, 128), rng.integers(0, 2, 128)
    Q[np.arange(128), axis] = np.where(side == 0, near, np.float32(1) - near).astype(np.float32)
    assert in_cell(Q, lo, period).all()
    return P, Q


def edge_case():
    """(P, Q, radii): 900 uniform points of the non-dyadic cell, 20 of them with a NaN in z (the open axis; the box of the set
    ignores them), 40 of them copies of one point; queries: that point, in-cell ones, ones outside the cell on either periodic
    axis (by an ulp and by far), ones with a NaN; radii with NaN, +-inf, 0 and negative entries among ordinary ones."""
    lo, period = CELL
    P = uniform_in(lo, period, 900, 89, open_width=0.3)
    rng = np.random.default_rng(90)
    rows = rng.choice(len(P), 60, replace=False)
    P[rows[:20], 2] = np.nan
    P[rows[20:]] = np.float32([0.11, 0.39, 2.1])
    Q = uniform_in(lo, period, 64, 91, open_width=0.3)
    Q[0] = np.float32([0.11, 0.39, 2.1])
    hi = (lo + period).astype(np.float32)
    Q[1, 0] = np.nextafter(lo[0], np.float32(-1))  # an ulp below lo
    Q[2, 1] = np.nextafter(np.nextafter(hi[1], np.float32(9)), np.float32(9))  # just above lo + L
    Q[3, 0] = np.float32(7.5)
    Q[4, 1] = np.float32(-5)
    Q[5, 0] = lo[0]  # ON the faces: in the cell
    Q[6, 1] = hi[1] if np.float32(hi[1] - lo[1]) <= period[1] else np.nextafter(hi[1], np.float32(-9))
    Q[7, 0], Q[8, 1], Q[9, 2] = np.nan, np.nan, np.nan
    Q[10, 2] = np.float32(50)  # far away on the open axis: an ordinary row
    radii = np.full(len(Q), 0.05, np.float32)
    radii[11:18] = np.float32([np.nan, np.inf, -np.inf, 0, -1, FLT_MAX, 1e-30])
    return P, np.ascontiguousarray(Q), radii
