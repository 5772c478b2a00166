"""What TrueKNN.radius_knn (tknnRadiusKnn) must return, restated in numpy, and the cases its tests share.  No tests here.

Row j is the row radius_spec.radius_rows gives q_j at its radius -- brute force over every pair, the fp32 distance
sqrt((dx*dx + dy*dy) + dz*dz) <= r, ascending in (distance, index) --, with the skipped point removed, cut after k entries
and padded with idx -1 / dist +inf; counts[j] = min(k, the row's length).  A row whose radius is NaN, not finite or <= 0 is
empty.  No kd-tree, no gate, no traversal: the spec cannot share a mistake with the kernels.
"""
import numpy as np

import query_spec as qs
import radius_spec as rs

K_ALL = (1, 5, 16, 17, 32, 33, 48, 49, 64)  # every list size of the team kernel (16, 32, 48, 64 entries) and both sides of each boundary
MAX_N, MAX_M = 4096, 600  # the GPU tests stay at or below these


def cut_rows(rows, k, skip=None):
    """CSR rows of radius_spec.radius_rows as dict(idx (m,k) int32, dist (m,k) float32, counts (m,) int32, lengths (m,) int64):
    each row without the entry skip[j] names (a negative value: nothing), its first k entries, the tail padded; lengths are the
    rows' lengths before the cut."""
    m = len(rows["lengths"])
    idx = np.full((m, k), -1, np.int32)
    dist = np.full((m, k), np.inf, np.float32)
    counts = np.zeros(m, np.int32)
    lengths = np.zeros(m, np.int64)
    for j in range(m):
        a, b = rows["offsets"][j], rows["offsets"][j + 1]
        i, d = rows["idx"][a:b], rows["dist"][a:b]
        if skip is not None and skip[j] >= 0:
            keep = i != skip[j]
            i, d = i[keep], d[keep]
        c = min(k, len(i))
        idx[j, :c], dist[j, :c], counts[j], lengths[j] = i[:c], d[:c], c, len(i)
    return {"idx": idx, "dist": dist, "counts": counts, "lengths": lengths}


def knn_rows(P, Q, k, radius=None, radii=None, skip=None, ids=None):
    """The spec's rows of a call; exactly one of radius and radii (per query) is given."""
    assert (radius is None) != (radii is None)
    if radii is None:
        return cut_rows(rs.radius_rows(P, Q, radius, ids=ids), k, skip)
    radii = np.asarray(radii, np.float32)
    Q = np.asarray(Q, np.float32)
    m = len(Q)
    skip = np.full(m, -1, np.int64) if skip is None else np.asarray(skip)
    out = {"idx": np.full((m, k), -1, np.int32), "dist": np.full((m, k), np.inf, np.float32), "counts": np.zeros(m, np.int32),
           "lengths": np.zeros(m, np.int64)}
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(radii) & (radii > 0)
    for r in np.unique(radii[valid]):
        sel = np.flatnonzero(valid & (radii == r))
        part = cut_rows(rs.radius_rows(P, Q[sel], r, ids=ids), k, skip[sel])
        for key in out:
            out[key][sel] = part[key]
    return out


def knn_set(name):
    """(P, Q, r0) of query_spec.make_set(name) within the GPU tests' sizes.  Of a larger set: the MAX_N points nearest its first
    point in the Chebyshev sense -- a cube cut out around a point of the set, so the density, and with it the row lengths at r0,
    stay the set's own, and in the clustered set the cube holds whole clusters.  Of more queries: the MAX_M / 2 nearest that
    point (rows as long as the set gives) and every s-th of the others (mostly outside the cube: empty rows)."""
    P, Q, r0 = qs.make_set(name)
    centre = P[0]
    if len(P) > MAX_N:
        keep = np.sort(np.argsort(np.abs(P - centre).max(axis=1), kind="stable")[:MAX_N])
        P = np.ascontiguousarray(P[keep])
    if len(Q) > MAX_M:
        near = np.argsort(np.abs(Q - centre).max(axis=1), kind="stable")
        rest = np.sort(near[MAX_M // 2:])
        pick = np.concatenate([np.sort(near[:MAX_M // 2]), rest[:: -(-len(rest) // (MAX_M // 2))]])
        Q = np.ascontiguousarray(Q[pick])
    return P, Q, r0


def set_radius(r0, factor):
    return np.float32(np.float32(r0) * np.float32(factor))


def set_rows(name, factor):
    """(P, Q, r, the full CSR rows) of a set at r = r0 * factor, computed once."""
    P, Q, r0 = knn_set(name)
    r = set_radius(r0, factor)
    return P, Q, r, rs.rows_of(("knn-set", name, factor), lambda: rs.radius_rows(P, Q, r))


def set_case_is_sharp(name, factor, k):
    """Whether the case has a row shorter than k and a row longer than k: a kernel that never cuts, or always fills, fails it."""
    lengths = set_rows(name, factor)[3]["lengths"]
    return bool((lengths < k).any() and (lengths > k).any())


# radius_spec.SET_NAMES x SET_FACTORS x K_ALL, without the combinations brute force shows to have no row shorter than k or no row
# longer than k (tests/test_radius_knn_expectations.py holds the list against set_case_is_sharp, both ways)
SET_CASES = (
    ("uniform", 1, 1), ("uniform", 3, 1), ("uniform", 3, 5), ("copies", 1, 1), ("copies", 3, 1), ("copies", 3, 5),
    ("duplicates", 1, 1), ("duplicates", 3, 5), ("duplicates", 3, 16), ("duplicates", 3, 17),
    ("planar", 1, 1), ("planar", 3, 1), ("planar", 3, 5), ("planar", 3, 16), ("planar", 3, 17),
    ("scale_down", 1, 1), ("scale_down", 3, 1), ("scale_down", 3, 5), ("scale_up", 1, 1), ("scale_up", 3, 1), ("scale_up", 3, 5),
)
# At r0 x 3 no set of this size has a row of more than 30 entries, so the list above never reaches the lists of 32, 48 and 64
# entries.  The dense case does, at every k of K_ALL: uniform_case()'s points, queries from a cube that overlaps theirs by 0.2
# on every side, and a radius that gives rows of some 130 entries well inside and of 0 .. 64 at the faces, edges and corners.
DENSE_RADIUS = np.float32(0.2)

LATTICE_K = (1, 3, 6, 7)
CHUNK_K = (16, 17, 64)
FALLBACK_K = (5, 17, 64)


def dense_rows():
    """(P, Q, r, the full CSR rows) of the dense case, computed once."""
    P = uniform_case()[0]
    Q = np.random.default_rng(63).random((256, 3), dtype=np.float32) * np.float32(1.4) - np.float32(0.2)
    return P, Q, DENSE_RADIUS, rs.rows_of(("knn-dense",), lambda: rs.radius_rows(P, Q, DENSE_RADIUS))


def uniform_case():
    """(P, Q): 4 096 uniform points and 256 queries; at radius 4.0 every point is in reach of every query."""
    from owlraytracing_amd import datasets

    return datasets.uniform3d(4096, seed=61), np.random.default_rng(62).random((256, 3), dtype=np.float32)
