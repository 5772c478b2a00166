"""What TrueKNN.local_pca (tknnLocalPca, include/owlknn_pca.h) must give, restated in numpy, the tolerances its outputs are held to,
the device's eigen-solver restated in float32, and the cases its tests share.  No tests here.

The neighbourhood N_j (`members`) by brute force over all pairs, with the fp32 distance sqrt((dx*dx + dy*dy) + dz*dz) and ties by
name (the id where ids are given, the row otherwise) -- the header's definition spelled out on its own, so that
test_pca_expectations.py can hold it against radius_spec, knn_spec and radius_knn_spec, whose rows it must equal as sets:
  * radius only: dist <= r; with the set's own points the point itself is in unless skip; a coinciding duplicate always stays;
  * k, external queries: the first k of the points at a finite distance in (distance, name) order; with a radius: those <= r;
  * k, own points: the point itself (if its coordinates are finite) and the first k - 1 of the OTHER points (told by name) in that
    order, clipped by the radius; with skip: the first k of the other points, the point itself out;
  * a NaN on either side: not a neighbour.  Batch labels play no part.
The moments, the centroid, the covariance and numpy's eigh in float64 from the fp32 offsets d = p - q (`want`).

The tolerances are derived, not measured.  u = 2^-24, R = R_j the largest float64 length of an offset of the row, so every
|d_a| <= R.  An fp32 sum of len terms t in any order errs by at most (len - 1) u sum|t| to first order; each product, quotient
and sum adds one rounding.
  centroid.  S1_a errs by (len - 1) u len R; divided by len: (len - 1) u R, plus the quotient's rounding u R; the sum q_a + mean_a
      adds u |c_a|.  Together u (len R + |c_a|) to first order.  Held to 2 u ((len + 3) R + |c_a|): the factor 2 for second-order
      terms and any contraction, the 3 for the (1 + u) factors left out above.
  covariance.  Each product d_a d_b carries u R^2, their sum errs by (len - 1) u len R^2 + len u R^2; divided by len and rounded:
      (len + 1) u R^2.  A mean errs by len u R (above), so mean_a mean_b errs by 2 len u R^2 + u R^2; the difference adds u R^2.
      Together (3 len + 3) u R^2 to first order.  Held to 2 u (3 len + 12) R^2, which is not below it.
  The floor 1e-37 covers denormal results.
The eigen outputs are held to these and to the solver constant E below (test_pca_gpu.py says how).

E cannot be derived for an iteration whose operation count depends on the matrix, so it is MEASURED -- on the CPU, against
`jacobi32`, never against the device: `solver_defects` runs jacobi32 over the float64 covariances (rounded to fp32) of every case
below and gives, in units of u, the largest residual |C v - lambda v|_inf / |C|_F, the largest orthonormality defect |V V^T - I|
and the largest eigenvalue error against eigvalsh / |C|_F.  E is 4 x the largest of the three, rounded up to a power of two;
test_pca_expectations.py holds jacobi32 to E / 4 on every case.  The margin of 4 covers what the device may legitimately do
differently -- FMA contraction, another rounding of division and rsqrt: one rounding per operation, not more operations.  A wrong
rotation errs by about |C|, a million times more.
"""
import numpy as np

from owlraytracing_amd import datasets
from owlraytracing_amd.datasets import pad_to_3d

import knn_spec as ks
import reduce_spec as rd

U = 2.0 ** -24
SWEEPS = 6         # kPcaSweeps
MIN_POINTS = 3
GAP = 0.05         # the normal is compared on rows with l1 - l0 >= GAP * l2 ...
GAP_CAP = 0.05     # ... and at most this share of a case's rows with len >= min_points may be left out
SOLVER_OBSERVED = 15.02  # the largest of solver_defects() over all cases, in units of u: the orthonormality defect (sphere1025); the
                         # residual reaches 4.35 and the eigenvalue error 4.47 (plane4200)
E = 64.0           # 4 x SOLVER_OBSERVED = 60.1, rounded up to a power of two
K_ALL = (2, 3, 16, 64)
OUTPUTS = ("counts", "centroid", "cov", "eigenvalues", "eigenvectors", "normals", "curvature")


# ---- N_j -----------------------------------------------------------------------------------------------------------------------------
def members(P, Q, radius=None, k=None, skip_self=False, ids=None, block=256):
    """N_j in CSR form: dict(offsets (m+1,) int64, idx (total,) int64 rows of P ascending inside a row, lengths (m,) int64).
    Q None: the rows of P are the queries."""
    assert radius is not None or k is not None
    P = pad_to_3d(np.asarray(P, np.float32))
    own = Q is None
    Qa = P if own else pad_to_3d(np.asarray(Q, np.float32))
    assert own or not skip_self
    n, m = len(P), len(Qa)
    names = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    kk = None if k is None else (k - 1 if own and not skip_self else k)
    assert kk is None or kk >= 1
    r = None if radius is None else np.float32(radius)
    lengths = np.zeros(m, np.int64)
    rows = []
    for s in range(0, m, block):
        with np.errstate(invalid="ignore", over="ignore"):
            diff = P[None, :, :] - Qa[s:s + block, None, :]
            x, y, z = diff[..., 0], diff[..., 1], diff[..., 2]
            d = np.sqrt(((x * x) + (y * y)) + (z * z), dtype=np.float32)
            near = np.isfinite(d) if r is None else d <= r  # (NaN <= r is False)
        for t in range(d.shape[0]):
            j = s + t
            if kk is None:
                c = np.flatnonzero(near[t])
                if skip_self:
                    c = c[c != j]
            else:
                other = np.isfinite(d[t])
                if own:
                    other &= names != names[j]
                c = np.flatnonzero(other)
                if len(c) > kk:
                    c = c[d[t, c] <= np.partition(d[t, c], kk - 1)[kk - 1]]
                c = c[np.lexsort((names[c], d[t, c]))][:kk]
                c = c[near[t, c]]
                if own and not skip_self and np.isfinite(d[t, j]):
                    c = np.concatenate([c, [j]])
                c = np.sort(c)
            lengths[j] = len(c)
            rows.append(c.astype(np.int64))
    out = {"offsets": np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), "idx": np.concatenate(rows) if rows else np.zeros(0, np.int64),
           "lengths": lengths}
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- moments, covariance, eigh in float64 ---------------------------------------------------------------------------------------------
def cov_matrix(cov6):
    """(m, 3, 3) from (m, 6) xx, xy, xz, yy, yz, zz."""
    c = np.asarray(cov6)
    return np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], axis=1)


def want(P, Q, mem, min_points=MIN_POINTS):
    """What the call must give for the rows `mem`, in float64: dict(counts, len, centroid (m,3), cov (m,6), R (m,), tol_centroid
    (m,3), tol_cov (m,), eigenvalues (m,3), normal (m,3: numpy's eigenvector of the smallest), normF (m,: |C|_F), solved (m,) bool:
    len >= min_points, gap (m,) bool: the rows the normal is compared on)."""
    P = pad_to_3d(np.asarray(P, np.float32))
    Qa = P if Q is None else pad_to_3d(np.asarray(Q, np.float32))
    m = len(Qa)
    ln = mem["lengths"]
    rowid = np.repeat(np.arange(m), ln)
    d = (P[mem["idx"]] - Qa[rowid]).astype(np.float64)  # the fp32 offsets
    S1 = np.stack([np.bincount(rowid, weights=d[:, a], minlength=m) for a in range(3)], axis=1)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    S2 = np.stack([np.bincount(rowid, weights=d[:, a] * d[:, b], minlength=m) for a, b in pairs], axis=1)
    R = np.zeros(m)
    np.maximum.at(R, rowid, np.sqrt((d * d).sum(axis=1)))
    lf = np.maximum(ln, 1).astype(np.float64)[:, None]
    mean = S1 / lf
    with np.errstate(invalid="ignore"):
        centroid = np.where(ln[:, None] > 0, Qa.astype(np.float64) + mean, 0.0)
    cov = S2 / lf - np.stack([mean[:, a] * mean[:, b] for a, b in pairs], axis=1)
    lnf = ln.astype(np.float64)
    tol_centroid = 2.0 * U * ((lnf + 3.0)[:, None] * R[:, None] + np.abs(centroid)) + 1e-37
    tol_cov = 2.0 * U * (3.0 * lnf + 12.0) * R * R + 1e-37
    solved = ln >= min_points
    lam, vec = np.linalg.eigh(cov_matrix(cov))
    lam = np.where(solved[:, None], lam, 0.0)
    normal = np.where(solved[:, None], vec[:, :, 0], 0.0)
    normF = np.sqrt((cov_matrix(cov) ** 2).sum(axis=(1, 2)))
    gap = solved & (lam[:, 1] - lam[:, 0] >= GAP * lam[:, 2]) & (lam[:, 2] > 0)
    return {"counts": ln.astype(np.int64), "len": ln, "centroid": centroid, "cov": cov, "R": R, "tol_centroid": tol_centroid, "tol_cov": tol_cov,
            "eigenvalues": lam, "normal": normal, "normF": normF, "solved": solved, "gap": gap}


# ---- the device's solver, operation for operation, in float32 ---------------------------------------------------------------------------
def _rotate(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q):
    """pca_rotate over arrays: every line one fp32 operation per element, the rows with apq == 0 left as they are."""
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        live = apq != 0
        theta = (aqq - app) / (f(2) * apq)
        root = np.sqrt(theta * theta + f(1), dtype=np.float32)
        t = np.where(theta >= 0, f(1), f(-1)) / (np.abs(theta) + root)
        c = f(1) / np.sqrt(t * t + f(1), dtype=np.float32)
        sn = t * c
        h = t * apq
        new = (app - h, aqq + h, np.zeros_like(apq), c * arp - sn * arq, sn * arp + c * arq, c * v0p - sn * v0q, sn * v0p + c * v0q,
               c * v1p - sn * v1q, sn * v1p + c * v1q, c * v2p - sn * v2q, sn * v2p + c * v2q)
    old = (app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)
    return tuple(np.where(live, a, b).astype(np.float32) for a, b in zip(new, old))


def jacobi32(cov6):
    """pca_eig3 over the rows of cov6 (m, 6) float32: (eigenvalues (m,3) ascending, eigenvectors (m,3,3), row i belonging to
    eigenvalue i), float32."""
    f = np.float32
    cv = np.ascontiguousarray(cov6, np.float32)
    m = len(cv)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        scale = np.abs(cv).max(axis=1).astype(np.float32)
        ok = (scale > 0) & (scale <= np.finfo(np.float32).max)
        scale = np.where(ok, scale, f(0)).astype(np.float32)
        inv = f(1) / np.where(ok, scale, f(1)).astype(np.float32)
        a = np.where(ok[:, None], cv * inv[:, None], f(0)).astype(np.float32)
    a00, a01, a02, a11, a12, a22 = (a[:, i].copy() for i in range(6))
    one, zero = np.ones(m, np.float32), np.zeros(m, np.float32)
    v00, v01, v02, v10, v11, v12, v20, v21, v22 = one, zero, zero, zero, one.copy(), zero, zero, zero, one.copy()
    for _ in range(SWEEPS):
        a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21 = _rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
        a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22 = _rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
        a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22 = _rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
    lam = [a00 * scale, a11 * scale, a22 * scale]
    col = [[v00, v10, v20], [v01, v11, v21], [v02, v12, v22]]  # col[c]: the eigenvector of lam[c]

    def order(i, j):
        sw = lam[j] < lam[i]
        lam[i], lam[j] = np.where(sw, lam[j], lam[i]), np.where(sw, lam[i], lam[j])
        for t in range(3):
            col[i][t], col[j][t] = np.where(sw, col[j][t], col[i][t]), np.where(sw, col[i][t], col[j][t])

    order(0, 1), order(1, 2), order(0, 1)
    return np.stack(lam, axis=1).astype(np.float32), np.stack([np.stack(c, axis=1) for c in col], axis=1).astype(np.float32)


def defects(cov6, lam, vec):
    """Of eigenpairs (lam (m,3), vec (m,3,3) rows) against the symmetric matrices cov6, evaluated in float64: dict(residual (m,):
    max |C v - lambda v|_inf / |C|_F, ortho (m,): max |V V^T - I|, normF (m,)); rows with |C|_F = 0 have residual 0."""
    C = cov_matrix(np.asarray(cov6, np.float64))
    lam, V = np.asarray(lam, np.float64), np.asarray(vec, np.float64)
    normF = np.sqrt((C ** 2).sum(axis=(1, 2)))
    res = np.abs(np.einsum("mab,mib->mia", C, V) - lam[:, :, None] * V).max(axis=(1, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        res = np.where(normF > 0, res / normF, 0.0)
    ortho = np.abs(np.einsum("mia,mja->mij", V, V) - np.eye(3)[None]).max(axis=(1, 2))
    return {"residual": res, "ortho": ortho, "normF": normF}


def sign32(normal, Q, viewpoint=None):
    """The sign rule recomputed in fp32 from a written normal (m,3): the quantity that must not be negative -- the component of
    largest magnitude, the first among equals, or with a viewpoint s = (n_x v_x + n_y v_y) + n_z v_z, v = viewpoint - q."""
    nrm = np.asarray(normal, np.float32)
    if viewpoint is None:
        big = nrm[:, 0].copy()
        for a in (1, 2):
            take = np.abs(nrm[:, a]) > np.abs(big)
            big = np.where(take, nrm[:, a], big)
        return big
    v = (np.asarray(viewpoint, np.float32)[None, :] - np.asarray(Q, np.float32)).astype(np.float32)
    return ((nrm[:, 0] * v[:, 0] + nrm[:, 1] * v[:, 1]) + nrm[:, 2] * v[:, 2]).astype(np.float32)


def curvature32(lam):
    """The header's formula on written eigenvalues (m,3), in fp32."""
    lam = np.asarray(lam, np.float32)
    total = ((lam[:, 0] + lam[:, 1]) + lam[:, 2]).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(total > 0, np.maximum(lam[:, 0], np.float32(0)) / np.where(total > 0, total, np.float32(1)), np.float32(0)).astype(np.float32)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def _shape(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "plane":  # a noisy tilted plane over the unit square
        xy = rng.random((n, 2))
        z = 0.3 * xy[:, 0] + 0.2 * xy[:, 1] + 0.1 + 0.002 * rng.standard_normal(n)
        return np.column_stack([xy, z]).astype(np.float32)
    if kind == "sphere":
        v = rng.standard_normal((n, 3))
        return (0.5 + 0.5 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    assert kind == "cube"
    return datasets.uniform3d(n, seed=seed)


def _radius20(kind, n):
    """A radius with about 20 points within it (the whole of a set that small)."""
    if kind == "plane":
        r = np.sqrt(20.0 / (np.pi * n))
    elif kind == "sphere":
        r = np.sqrt(20.0 / n)
    else:
        r = (15.0 / (np.pi * n)) ** (1.0 / 3.0)
    return np.float32(min(r, 0.8))


def _queries(P, seed, count=48):
    """Jittered copies of points, some points themselves, two far queries."""
    rng = np.random.default_rng(seed)
    clean = P[~np.isnan(P).any(axis=1)]
    near = clean[rng.integers(0, len(clean), count)] + (rng.random((count, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(0.02)
    return np.concatenate([near, clean[:4], np.float32([[3, 3, 3], [-2, 0.5, 0.5]])]).astype(np.float32)


SHAPES = ("plane", "sphere", "cube")
SIZES = (15, 1025, 4200)  # no pyramid (the lane kernel alone); the leaf-block edge; past 64^2 points: a third level
SHAPE_CASES = tuple("%s%d" % (kind, n) for n in SIZES for kind in SHAPES)
SPECIAL_CASES = ("coincide", "collinear", "ties", "nan", "long")
CASE_NAMES = SHAPE_CASES + SPECIAL_CASES


def _make(name):
    ids = None
    modes = ("ext", "own", "own_skip")
    hoods = None
    for kind in SHAPES:
        if name.startswith(kind):
            n = int(name[len(kind):])
            P = _shape(kind, n, 300 + n + SHAPES.index(kind))
            Q = _queries(P, 400 + n)
            r = _radius20(kind, n)
            break
    else:
        if name == "coincide":  # R_j = 0 and the name rule at distance 0
            P = np.tile(np.float32([[0.3, 0.7, 0.2]]), (300, 1))
            Q = np.concatenate([P[:2], np.float32([[0.3, 0.7, 0.25], [0.9, 0.1, 0.1]])])
            r = np.float32(0.1)
        elif name == "collinear":
            t = np.random.default_rng(501).random(200)
            P = (np.float64([0.1, 0.2, 0.3])[None, :] + t[:, None] * np.float64([0.6, 0.3, -0.2])[None, :]).astype(np.float32)
            Q = _queries(P, 502, count=24)
            r = np.float32(0.08)
        elif name == "ties":  # a lattice of spacing 1/8, exact in fp32: distances exactly r, ties at the k-th place at every k; ids reverse the rows
            g = np.arange(7, dtype=np.float32) / np.float32(8)
            P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
            P = P[np.random.default_rng(503).permutation(len(P))]
            ids = (len(P) - 1 - np.arange(len(P))).astype(np.int32)
            Q = np.concatenate([P[::9], P[::11] + np.float32(1.0 / 16)]).astype(np.float32)  # nodes and cell centres
            r = np.float32(1.0 / 8)
        elif name == "nan":
            P, Q = (np.array(a) for a in ks.nan_case())
            r = np.float32(0.2)
        elif name == "long":  # rows of half the set: more boxes inside the sphere than a team's range list holds
            c = rd.case("n66000")
            P, Q, r = c["P"], c["Q"], c["radii"]["half"]
            modes = ("ext",)
            hoods = (("r", r, None), ("rk", r, 64))
        else:
            raise KeyError(name)
    if hoods is None:
        hoods = (("r", r, None),) + tuple(("k", None, k) for k in K_ALL) + (("rk", r, 16),)
    return {"P": np.ascontiguousarray(P, np.float32), "Q": np.ascontiguousarray(Q, np.float32), "ids": ids, "modes": modes, "hoods": hoods, "radius": r}


_cache = {}


def case(name):
    """A named set, made once and shared (do not write to it): dict(P, Q, ids, modes, hoods: (label, radius, k) triples, radius)."""
    if ("case", name) not in _cache:
        c = _make(name)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[("case", name)] = c
    return _cache[("case", name)]


def hood_label(hood):
    return hood[0] if hood[2] is None else "%s%d" % (hood[0], hood[2])


def want_of(name, mode, hood, with_ids=False):
    """(members, want) of a case in a mode ("ext", "own", "own_skip") at a neighbourhood (label, radius, k), made once and shared.
    with_ids: ties by the case's ids."""
    key = ("want", name, mode, hood_label(hood), with_ids)
    if key not in _cache:
        c = case(name)
        Q = c["Q"] if mode == "ext" else None
        mem = members(c["P"], Q, radius=hood[1], k=hood[2], skip_self=mode == "own_skip", ids=c["ids"] if with_ids else None)
        w = want(c["P"], Q, mem)
        for a in w.values():
            a.setflags(write=False)
        _cache[key] = (mem, w)
    return _cache[key]


def all_combinations():
    """(name, mode, hood) of everything the GPU tests run."""
    for name in CASE_NAMES:
        c = case(name)
        for mode in c["modes"]:
            for hood in c["hoods"]:
                if mode == "own" and hood[2] is not None and hood[2] < 2:
                    continue
                yield name, mode, hood


def solver_defects(names=CASE_NAMES):
    """jacobi32 over the float64 covariances, rounded to fp32, of every combination of `names`: the three maxima in units of u
    (residual, ortho, eigenvalue error against eigvalsh / |C|_F)."""
    worst = np.zeros(3)
    for name, mode, hood in all_combinations():
        if name not in names:
            continue
        w = want_of(name, mode, hood, with_ids=case(name)["ids"] is not None)[1]
        c32 = w["cov"][w["solved"]].astype(np.float32)
        if not len(c32):
            continue
        lam, vec = jacobi32(c32)
        dfc = defects(c32, lam, vec)
        ref = np.linalg.eigvalsh(cov_matrix(c32.astype(np.float64)))
        with np.errstate(invalid="ignore", divide="ignore"):
            lerr = np.where(dfc["normF"] > 0, np.abs(lam.astype(np.float64) - ref).max(axis=1) / dfc["normF"], 0.0)
        worst = np.maximum(worst, [dfc["residual"].max() / U, dfc["ortho"].max() / U, lerr.max() / U])
    return worst
