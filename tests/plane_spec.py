"""include/owlknn_plane.h (tknnSegmentPlane) restated in numpy: fp32 with every product and sum rounded on its own (numpy's float32
arithmetic rounds each operation; nothing here is contracted), brute force over all active rows, no tree.  No tests here.

The trials, their statuses and counts, the best trial, the stop rule, the mask and the rows are exact.  The refit's plane is the
header's to a tolerance (the device sums its fp64 moments in its own fixed order): refit() gives this restatement's plane and the
header's bound; what follows from the fp32 plane the device reports is exact again (evaluate())."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_spec  # noqa: E402  (the sample of a trial: tknnRansac's)

OK, DUPLICATE, DEGENERATE, ANGLE = 0, 1, 2, 3
STATUS = ("ok", "duplicate", "degenerate", "angle")
BATCH = 1024
F = np.float32
U24 = 2.0 ** -24


# ---- the active rows ----------------------------------------------------------------------------------------------------------------
def active_rows(P, active=None):
    """A: the rows with three finite coordinates and (active is None or active[row] != 0), ascending."""
    P = np.asarray(P, F)
    keep = np.isfinite(P).all(axis=1)
    if active is not None:
        keep &= np.asarray(active) != 0
    return np.flatnonzero(keep)


# ---- the trials ---------------------------------------------------------------------------------------------------------------------
def unit_axis(axis):
    """The axis as the trials take it (double, rounded to fp32 once), or None for no axis or an all-zero one."""
    if axis is None:
        return None
    x, y, z = (float(F(v)) for v in axis)
    if x == 0.0 and y == 0.0 and z == 0.0:
        return None
    length = math.sqrt((x * x + y * y) + z * z)
    return np.array([x / length, y / length, z / length], np.float64).astype(F)


def trial_planes(P, A, seed, trials, axis=None, min_cos=None):
    """(status (t,), normal (t,3) fp32, anchor (t,3) fp32, idx (t,3)) of the trials over the active rows A of P."""
    P, trials = np.asarray(P, F), np.asarray(trials)
    c, nt = len(A), len(trials)
    idx, drawn = global_spec.samples(seed, trials, 3, c)
    status = np.where(drawn, OK, DUPLICATE)
    idx = np.where(drawn[:, None], idx, 0)
    p0, p1, p2 = (P[A[idx[:, s]]] for s in range(3))
    with np.errstate(all="ignore"):
        e1, e2 = p1 - p0, p2 - p0
        g = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        l1 = (e1[:, 0] * e1[:, 0] + e1[:, 1] * e1[:, 1]) + e1[:, 2] * e1[:, 2]
        l2 = (e2[:, 0] * e2[:, 0] + e2[:, 1] * e2[:, 1]) + e2[:, 2] * e2[:, 2]
        g2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        good = np.isfinite(g2) & (g2 > F(2.0 ** -40) * (l1 * l2))
        q = np.sqrt(g2)
        normal = g / q[:, None]
    assert normal.dtype == F and g2.dtype == F
    status = np.where((status == OK) & ~good, DEGENERATE, status)
    unit = unit_axis(axis)
    if unit is not None:
        with np.errstate(all="ignore"):
            dot = np.abs((normal[:, 0] * unit[0] + normal[:, 1] * unit[1]) + normal[:, 2] * unit[2])
        assert dot.dtype == F
        status = np.where((status == OK) & ~(dot >= F(min_cos)), ANGLE, status)
    normal = np.where((status == OK)[:, None], normal, F(0)).astype(F)
    anchor = np.where((status == OK)[:, None], p0, F(0)).astype(F)
    return status, normal, anchor, idx


def distances(normal, anchor, X):
    """The fp32 distance of the rows X (m,3) to the planes (t,3), (t,3): (t, m) fp32, NaN for a row that is not finite."""
    normal, anchor, X = np.asarray(normal, F).reshape(-1, 3), np.asarray(anchor, F).reshape(-1, 3), np.asarray(X, F)
    with np.errstate(all="ignore"):
        dx, dy, dz = (X[None, :, i] - anchor[:, None, i] for i in range(3))
        s = (normal[:, None, 0] * dx + normal[:, None, 1] * dy) + normal[:, None, 2] * dz
    assert s.dtype == F
    return np.abs(s)


def scores(P, A, normal, anchor, thr, chunk=None):
    """The inlier counts of the planes over the active rows."""
    X, out = np.asarray(P, F)[A], np.zeros(len(normal), np.int64)
    chunk = chunk or max(1, (1 << 22) // max(len(X), 1))
    for lo in range(0, len(normal), chunk):
        out[lo:lo + chunk] = (distances(normal[lo:lo + chunk], anchor[lo:lo + chunk], X) <= F(thr)).sum(axis=1)
    return out


# ---- the refit ----------------------------------------------------------------------------------------------------------------------
def jacobi(a):
    """plane_solve.h's plane_jacobi in Python floats (IEEE double, one rounding per operation): (diagonal, V)."""
    a = [[float(a[i][j]) for j in range(3)] for i in range(3)]
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(12):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = a[p][q]
            if apq == 0.0:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            a[p][p] = a[p][p] - t * apq
            a[q][q] = a[q][q] + t * apq
            a[p][q] = a[q][p] = 0.0
            arp, arq = a[r][p], a[r][q]
            a[r][p] = a[p][r] = c * arp - s * arq
            a[r][q] = a[q][r] = s * arp + c * arq
            for i in range(3):
                vip, viq = v[i][p], v[i][q]
                v[i][p] = c * vip - s * viq
                v[i][q] = s * vip + c * viq
    return [a[0][0], a[1][1], a[2][2]], v


def scene_centre(P):
    """The centre the moments are taken about: of the bounding box of the rows without a NaN, 0 on an axis where it is not finite."""
    P = np.asarray(P, F)
    ok = P[~np.isnan(P).any(axis=1)].astype(np.float64)
    if len(ok) == 0:
        return np.zeros(3)
    with np.errstate(all="ignore"):
        centre = 0.5 * (ok.min(axis=0) + ok.max(axis=0))
    return np.where(np.isfinite(centre), centre, 0.0)


def refit(P, rows, centre):
    """The refit's plane from the inlier rows: dict(normal, anchor fp32; tol_normal, tol_anchor: the header's bounds per component;
    gap = l1 - l0), or None where the refit stops."""
    X = np.asarray(P, F)[rows].astype(np.float64) - centre
    m = len(X)
    if m < 1:
        return None
    mean = X.sum(axis=0) / m
    S2 = X.T @ X
    cov = S2 / m - np.outer(mean, mean)
    if not np.isfinite(cov).all():
        return None
    lam, v = jacobi(cov)
    order = sorted(range(3), key=lambda i: (lam[i], i))
    l0, l1, l2 = (lam[i] for i in order)
    if not l1 - l0 > 2.0 ** -40 * l2:
        return None
    vec = np.array([v[i][order[0]] for i in range(3)])
    vec = vec / math.sqrt((vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2])
    anchor = mean + centre
    finite = np.asarray(P, F)[np.isfinite(np.asarray(P, F)).all(axis=1)].astype(np.float64)
    R = 0.5 * float(np.linalg.norm(finite.max(axis=0) - finite.min(axis=0)))
    tol_normal = 2.0 ** -23 + 6.0 * m * 2.0 ** -52 * R * R / (l1 - l0)
    tol_anchor = 2.0 ** -23 * max(float(np.abs(anchor).max()), R) + m * 2.0 ** -52 * R
    return dict(normal=vec.astype(F), anchor=anchor.astype(F), tol_normal=tol_normal, tol_anchor=tol_anchor, gap=l1 - l0)


# ---- the outputs --------------------------------------------------------------------------------------------------------------------
def output_plane(normal, anchor, axis=None):
    """(plane (4,) float64, sign) of the fp32 plane, as plane_solve.h's plane_output."""
    n, a = [float(x) for x in np.asarray(normal, F)], [float(x) for x in np.asarray(anchor, F)]
    unit, sign = unit_axis(axis), 0.0
    if unit is not None:
        dot = (n[0] * float(unit[0]) + n[1] * float(unit[1])) + n[2] * float(unit[2])
        sign = 1.0 if dot > 0 else (-1.0 if dot < 0 else 0.0)
    for x in n:
        if sign == 0.0:
            sign = 1.0 if x > 0 else (-1.0 if x < 0 else 0.0)
    if sign == 0.0:
        sign = 1.0
    p = [sign * x for x in n]
    return np.array(p + [-((p[0] * a[0] + p[1] * a[1]) + p[2] * a[2])]), sign


def evaluate(P, A, normal, anchor, thr):
    """What follows from an fp32 plane, exactly: dict(rows: the inlier rows ascending; mask (n,) uint8; inliers; rmse: of the fp32
    distances squared and summed in double -- the device's sum is within (inliers + 2) * 2^-53 of it, relatively)."""
    P = np.asarray(P, F)
    d = distances(normal, anchor, P[A])[0]
    inl = d <= F(thr)
    rows = A[inl]
    mask = np.zeros(len(P), np.uint8)
    mask[rows] = 1
    d64 = d[inl].astype(np.float64)
    return dict(rows=rows.astype(np.int32), mask=mask, inliers=int(inl.sum()), rmse=math.sqrt(float((d64 * d64).sum()) / inl.sum()) if inl.any() else 0.0)


# ---- the call -----------------------------------------------------------------------------------------------------------------------
def segment(P, thr, max_trials, seed=0, confidence=1.0, active=None, axis=None, min_cos=None):
    """The call without its refit: dict(active = c, A, trials_run, batches, status (max_trials,) and inliers (max_trials,) int32 with -1
    where not run / not scored, status_counts (4,), best_trial, normal, anchor (fp32, of the best trial; zero when there is none),
    scored: the OK trials run)."""
    P = np.asarray(P, F)
    A = active_rows(P, active)
    c = len(A)
    status, inliers = np.full(max_trials, -1, np.int32), np.full(max_trials, -1, np.int32)
    normal, anchor = np.zeros((max_trials, 3), F), np.zeros((max_trials, 3), F)
    run, batches, best, best_trial = 0, 0, -1, -1
    while c >= 3 and run < max_trials:
        t = np.arange(run, min(run + BATCH, max_trials))
        st, nm, an, _ = trial_planes(P, A, seed, t, axis, min_cos)
        status[t], normal[t], anchor[t] = st, nm, an
        ok = t[st == OK]
        inliers[ok] = scores(P, A, normal[ok], anchor[ok], thr)
        run, batches = int(t[-1]) + 1, batches + 1
        for k in ok:  # most inliers, ties to the smaller trial
            if inliers[k] > best:
                best, best_trial = int(inliers[k]), int(k)
        f = max(best, 0) / c
        needed = math.inf
        if confidence < 1.0 and f > 0.0:
            miss = math.log(1.0 - f ** 3) if f < 1.0 else -math.inf
            needed = math.log(1.0 - confidence) / miss if miss < 0.0 else math.inf
        if run >= needed:
            break
    counts = np.array([(status[:run] == s).sum() for s in range(4)], np.int64)
    return dict(active=c, A=A, trials_run=run, batches=batches, status=status, inliers=inliers, status_counts=counts, best_trial=best_trial,
                normal=normal[best_trial] if best_trial >= 0 else np.zeros(3, F), anchor=anchor[best_trial] if best_trial >= 0 else np.zeros(3, F),
                scored=int(counts[OK]))


# ---- clouds -------------------------------------------------------------------------------------------------------------------------
def cube(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(F)


def plane_clutter(n, seed, share=0.5, noise=0.002):
    """A tilted plane through the unit cube carrying `share` of the rows, with noise, and uniform clutter."""
    rng = np.random.default_rng(seed)
    m = int(n * share)
    uv = rng.random((m, 2))
    on = np.stack([uv[:, 0], uv[:, 1], 0.3 + 0.2 * uv[:, 0] + 0.1 * uv[:, 1] + noise * rng.standard_normal(m)], axis=1)
    P = np.concatenate([on, rng.random((n - m, 3))])
    return P[rng.permutation(n)].astype(F)


def lattice():
    """17 x 9 x 9 points with coordinates k / 8: every difference, product and sum of an axis-aligned plane's distance is exact, points
    lie exactly at distance thr = 1/8 and block boxes end exactly on slab faces."""
    g = np.stack(np.meshgrid(np.arange(17), np.arange(9), np.arange(9), indexing="ij"), axis=-1).reshape(-1, 3)
    return (g / 8.0).astype(F)


def three_planes(n, seed, noise=0.002):
    """Three planes (z = 0.1, x = 0.2, y + z = 1.5) with 35, 25 and 15 percent of the rows, and clutter in [0, 1]^3."""
    rng = np.random.default_rng(seed)
    a, b, c = int(0.35 * n), int(0.25 * n), int(0.15 * n)
    u = rng.random((n, 2))
    e = noise * rng.standard_normal(n)
    P = rng.random((n, 3))
    P[:a] = np.stack([u[:a, 0], u[:a, 1], 0.1 + e[:a]], axis=1)
    P[a:a + b] = np.stack([0.2 + e[a:a + b], u[a:a + b, 0], u[a:a + b, 1]], axis=1)
    P[a + b:a + b + c] = np.stack([u[a + b:a + b + c, 0], 0.75 + 0.5 * (u[a + b:a + b + c, 1] - 0.5) + e[a + b:a + b + c], 0.75 - 0.5 * (u[a + b:a + b + c, 1] - 0.5)], axis=1)
    return P[rng.permutation(n)].astype(F)


TRIALS = BATCH + 7  # two batches, one partial
N3 = 16 * 64 * 64 + 17  # three pyramid levels, a ragged tail
PRUNE_THR = 0.01  # of the unit cube's edge: test_plane_gpu.py's pruning condition


def sorted_order(P):
    """prim_id of the tree over P (tests/lbvh_spec.py's rebuild): the caller's row of every sorted slot."""
    import lbvh_spec

    return lbvh_spec.build_points(np.asarray(P, F))["prim_id"]


def _half_mask(P):
    """Clears about half the rows: the whole sorted blocks 1, 2 and 5, all but one row of block 3, and every other row elsewhere."""
    order = sorted_order(P)
    active = np.ones(len(P), np.uint8)
    active[::2] = 0
    for b in (1, 2, 5):
        active[order[16 * b:16 * b + 16]] = 0
    active[order[48:63]] = 0
    active[order[63]] = 1
    return active


def _duplicates(n, seed):
    rng = np.random.default_rng(seed)
    P = cube(n, seed)
    dup = rng.choice(n, n // 10, replace=False)
    P[dup[1:]] = P[dup[0]]  # (one point many times: a sample with two of its copies is DEGENERATE often enough to be seen)
    return P


def _bad_rows(n, seed):
    rng = np.random.default_rng(seed)
    P = plane_clutter(n, seed)
    bad = rng.choice(n, 60, replace=False)
    P[bad[:20], rng.integers(0, 3, 20)] = np.nan
    P[bad[20:40], rng.integers(0, 3, 20)] = np.inf
    P[bad[40:], rng.integers(0, 3, 20)] = -np.inf
    return P


def _few_of_duplicates():
    """Four active rows of the duplicates cloud, two of them one point: a slot's eight draws collide often enough for DUPLICATE
    (c = 1025 never does: (2 / c)^8), and a sample with both twins is DEGENERATE."""
    P = _duplicates(1025, 5)
    _, inv, cnt = np.unique(P, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    twins, singles = np.flatnonzero(cnt[inv] > 1), np.flatnonzero(cnt[inv] == 1)
    a = twins[0]
    b = next(j for j in twins if inv[j] == inv[a] and j != a)
    active = np.zeros(len(P), np.uint8)
    active[[a, b, singles[0], singles[1]]] = 1
    return dict(P=P, thr=0.05, active=active)


CASES = {
    "n2": lambda: dict(P=cube(2, 1), thr=0.05),
    "n3": lambda: dict(P=cube(3, 2), thr=0.05),
    "n17": lambda: dict(P=cube(17, 3), thr=0.05),
    "n1025": lambda: dict(P=cube(1025, 4), thr=0.05),
    "cube65553": lambda: dict(P=cube(N3, 5), thr=PRUNE_THR),
    "plane_clutter": lambda: dict(P=plane_clutter(4113, 6), thr=0.01),
    "plane_clutter_refit": lambda: dict(P=plane_clutter(4113, 6), thr=0.01, refit_rounds=1),
    "plane_tight_refit": lambda: dict(P=plane_clutter(4113, 6), thr=0.003, refit_rounds=1),  # 1.5 sigma of the noise: a refit gains inliers
    "lattice": lambda: dict(P=lattice(), thr=0.125),
    "shifted": lambda: dict(P=(plane_clutter(4113, 6) + np.array([1000, -2000, 500], F)).astype(F), thr=0.01),
    "lattice_shifted": lambda: dict(P=(lattice() + np.array([1000, -2000, 500], F)).astype(F), thr=0.125),
    "duplicates": lambda: dict(P=_duplicates(1025, 5), thr=0.05),
    "duplicates_c4": _few_of_duplicates,
    "nan_inf": lambda: dict(P=_bad_rows(1025, 7), thr=0.01),
    "active_half": lambda: (lambda P: dict(P=P, thr=0.01, active=_half_mask(P)))(plane_clutter(1025, 8)),
    "wide": lambda: dict(P=cube(4113, 9), thr=2.0),
    "axis": lambda: dict(P=plane_clutter(4113, 6), thr=0.01, axis=(0.0, 0.0, 2.0), min_cos=0.99),
}
TRIAL_SEED = 7


@functools.lru_cache(maxsize=None)
def case(name):
    """(c, want): the case's inputs with the defaults filled in, and segment()'s answer; computed once and shared -- read only."""
    c = dict(active=None, axis=None, min_cos=None, refit_rounds=0, trials=TRIALS, seed=TRIAL_SEED, confidence=1.0)
    c.update(CASES[name]())
    c["P"] = np.ascontiguousarray(c["P"], F)
    want = segment(c["P"], c["thr"], c["trials"], c["seed"], c["confidence"], c["active"], c["axis"], c["min_cos"])
    for a in (c["P"], want["status"], want["inliers"], want["A"]):
        a.setflags(write=False)
    return c, want


def block_share(P, thr, normal, anchor):
    """The mean share of the tree's 16-point blocks whose box meets the slabs |n . (x - a)| <= thr (real arithmetic, float64)."""
    import lbvh_spec

    t = lbvh_spec.build_points(np.asarray(P, F))
    boxes = t["wide_boxes"][:int(t["wide_count"][0])].astype(np.float64)
    lo, hi = boxes[:, :3], boxes[:, 3:]
    n64, a64 = np.asarray(normal, np.float64), np.asarray(anchor, np.float64)
    share = []
    for n, a in zip(n64, a64):
        centre, half = 0.5 * (lo + hi) - a, 0.5 * (hi - lo)
        share.append(float((np.abs(centre @ n) <= thr + half @ np.abs(n)).mean()))
    return float(np.mean(share))
