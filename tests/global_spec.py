"""What TrueKNN.match_features (tknnFeatureMatch) and TrueKNN.ransac (tknnRansac) of include/owlknn_global.h must give, restated in
numpy: the literal fp32 distance of descriptor rows and its two smallest per row; the hash, the draws, the fp32 edge check, Kabsch by
numpy's SVD in float64, and -- because the device solves by Horn's quaternion and measures in fp32 -- the classification of every
(trial, record) and of every sample member into certain inlier, certain outlier and uncertain, with the bound derived below.  The
scenes the GPU tests use are made here, fixed by seed.  No tests here.

The bound E on |d_device - d_spec| for one trial (d_spec: the distance of T s and p in float64 under the spec's float64 T):
  * the two solvers agree on T up to (bR on the rotation's entries, bt on the translation's) of icp_spec.point_bound -- 64 eps64
    |H|_F / (sigma2 + sigma3), the gap of Horn's matrix -- taken four-fold for the sums of up to four terms about a centre that is
    not the sample's own;
  * the device rounds the rows of T to fp32: a relative 2^-24 per entry, |R_ij| <= 1;
  * so s' moves by at most (bR + 2^-24) * 3 A + bt + 2^-24 * |t|_max per coordinate, A the largest |coordinate| of the sources;
  * the transform's six fp32 operations per coordinate, none above 3 A + |t|_max in magnitude: 6 * 2^-24 * (3 A + |t|_max);
  * three coordinates: sqrt(3) times the sum of the above;
  * the subtraction, squares, sums and square root in fp32: at most 4 * 2^-24 relative on d, which matters at d about max_dist only:
    4 * 2^-24 * 2 max_dist.
Nothing of it is fitted to the device's output."""
import numpy as np

import icp_spec

STATUS = ("ok", "duplicate", "edge", "degenerate", "far")
OK, DUPLICATE, EDGE, DEGENERATE, FAR = range(5)
BATCH = 4096
U24 = 2.0 ** -24
SIGMA2_FLOOR = icp_spec.SIGMA2_FLOOR
SIGMA2_BAND = 2.0 ** 5  # a ratio sigma2 / sigma1 within this factor of the floor is left to neither side


# ---- feature matching ---------------------------------------------------------------------------------------------------------------
def match(A, B):
    """(best (m,) int32, best_d2, second_d2 (m,) float32) of the rows A against the rows B: acc = acc + t*t channel by channel in
    float32; rows with an entry that is not finite are left out on both sides."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    m, n = len(A), len(B)
    best, b1, b2 = np.full(m, -1, np.int32), np.full(m, np.inf, np.float32), np.full(m, np.inf, np.float32)
    rows_s = np.nonzero(np.isfinite(A).all(axis=1))[0]
    rows_t = np.nonzero(np.isfinite(B).all(axis=1))[0] if n else np.zeros(0, np.int64)
    if len(rows_s) == 0 or len(rows_t) == 0:
        return best, b1, b2
    a, b = A[rows_s], B[rows_t]
    acc = np.zeros((len(a), len(b)), np.float32)
    with np.errstate(all="ignore"):
        for c in range(A.shape[1]):
            t = a[:, c, None] - b[None, :, c]
            acc = acc + t * t
    first = np.argmin(acc, axis=1)  # the first minimum: the smaller row
    pick = np.arange(len(a))
    b1[rows_s] = acc[pick, first]
    best[rows_s] = rows_t[first]
    rest = acc.copy()
    rest[pick, first] = np.inf
    b2[rows_s] = rest.min(axis=1)
    return best, b1, b2


def filter_pairs(best_s, b1, b2, best_t=None, ratio=None):
    """The pairs match_features keeps: best >= 0, [mutual: best_t[best_s[i]] == i,] [best_d2 <= fl32(ratio^2) * second_d2 in fp32]."""
    keep = best_s >= 0
    if best_t is not None:
        keep &= best_t[np.maximum(best_s, 0)] == np.arange(len(best_s))
    if ratio is not None:
        with np.errstate(all="ignore"):
            keep &= b1 <= np.float32(float(ratio) ** 2) * b2
    rows = np.nonzero(keep)[0]
    return np.stack([rows, best_s[rows]], axis=1).astype(np.int32)


def fpfh_like(rng, rows):
    """Rows like an FPFH: 33 non-negative channels, three groups of 11 that sum to 100 each, many exact zeros."""
    w = rng.random((rows, 3, 11)) ** 4
    w[rng.random((rows, 3, 11)) < 0.5] = 0.0
    w[:, :, 0] += 1e-3
    return (100.0 * w / w.sum(axis=2, keepdims=True)).reshape(rows, 33).astype(np.float32)


# ---- the sample ---------------------------------------------------------------------------------------------------------------------
def _hash(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def samples(seed, trials, n, c):
    """(idx (len(trials), n) int64, ok (len(trials),) bool) of the trials: slot s draws a = 0 .. 7 until its index differs from
    every earlier slot's; ok False where a slot finds none (the trial is DUPLICATE; its idx row is then meaningless)."""
    with np.errstate(over="ignore"):
        t = np.asarray(trials, np.uint32)
        key = _hash(np.uint32(seed) + np.uint32(0x9E3779B9) * t)
        idx = np.zeros((len(t), n), np.int64)
        ok = np.ones(len(t), bool)
        for s in range(n):
            found = np.zeros(len(t), bool)
            for a in range(8):
                u = _hash(key ^ (np.uint32(0x85EBCA6B) * np.uint32(8 * s + a + 1)))
                i = ((u.astype(np.uint64) * np.uint64(c)) >> np.uint64(32)).astype(np.int64)
                fresh = ~found
                for e in range(s):
                    fresh &= idx[:, e] != i
                idx[fresh, s] = i[fresh]
                found |= fresh
            ok &= found
    return idx, ok


# ---- one trial ----------------------------------------------------------------------------------------------------------------------
def edges_ok(s, p, sim):
    """The edge check of one sample in float32."""
    if not sim > 0:
        return True
    sim = np.float32(sim)
    s, p = np.asarray(s, np.float32), np.asarray(p, np.float32)
    for i in range(len(s)):
        for j in range(i + 1, len(s)):
            a, b = s[i] - s[j], p[i] - p[j]
            ds = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
            dt = np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
            if not (ds >= sim * dt and dt >= sim * ds):
                return False
    return True


def kabsch(s, p):
    """(T 4 x 4 or None where degenerate, aux for icp_spec.point_bound, sigma2 / sigma1) of the rows s -> p in float64."""
    s, p = np.asarray(s, np.float64), np.asarray(p, np.float64)
    mus, mup = s.mean(axis=0), p.mean(axis=0)
    H = (s - mus).T @ (p - mup)
    U, S, Vt = np.linalg.svd(H)
    ratio = S[1] / S[0] if S[0] > 0 else 0.0
    if not S[1] > SIGMA2_FLOOR * S[0]:
        return None, None, ratio
    V = Vt.T
    det = np.sign(np.linalg.det(V @ U.T))
    R = V @ np.diag([1.0, 1.0, det]) @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, mup - R @ mus
    return T, dict(H=H, sigma=np.array([S[0], S[1], det * S[2]]), mu_s=mus, mu_p=mup), ratio


def dist64(T, s, p):
    q = np.asarray(s, np.float64) @ T[:3, :3].T + T[:3, 3]
    return np.sqrt(((q - np.asarray(p, np.float64)) ** 2).sum(axis=1))


def bound(T, aux, A, max_dist):
    """(E, bR, bt) of the docstring for one trial."""
    bR, bt = icp_spec.point_bound(aux, factor=4.0)
    tmax = np.abs(T[:3, 3]).max()
    moved = (bR + U24) * 3 * A + bt + U24 * tmax
    evaluated = 6 * U24 * (3 * A + tmax)
    return np.sqrt(3.0) * (moved + evaluated) + 4 * U24 * 2 * float(max_dist), bR, bt


def run_trials(S, P, pairs, n, max_dist, sim, seed, trials):
    """The spec's view of the trials: dict(status (t,), excluded (t,) bool: a sample-member check or the degeneracy rule is
    uncertain, the status is then the device's to say; T (t,4,4), bR, bt, E (t,); certain, uncertain (t,) int: the records that are
    inliers for certain / within E of max_dist, of the trials whose status is OK; certain_mask, uncertain_mask (t, c) bool;
    idx (t, n))."""
    S, P, pairs = np.asarray(S, np.float32), np.asarray(P, np.float32), np.asarray(pairs)
    s_all, p_all = S[pairs[:, 0]], P[pairs[:, 1]]
    c = len(pairs)
    md = float(np.float32(max_dist))
    A = float(np.abs(S).max()) if len(S) else 0.0
    trials = np.asarray(trials)
    idx, drawn = samples(seed, trials, n, c)
    nt = len(trials)
    out = dict(status=np.full(nt, -1), excluded=np.zeros(nt, bool), T=np.tile(np.eye(4), (nt, 1, 1)), bR=np.zeros(nt), bt=np.zeros(nt), E=np.zeros(nt),
               certain=np.zeros(nt, np.int64), uncertain=np.zeros(nt, np.int64), certain_mask=np.zeros((nt, c), bool),
               uncertain_mask=np.zeros((nt, c), bool), idx=idx)
    for k in range(nt):
        if not drawn[k]:
            out["status"][k] = DUPLICATE
            continue
        s, p = s_all[idx[k]], p_all[idx[k]]
        if not edges_ok(s, p, sim):
            out["status"][k] = EDGE
            continue
        T, aux, ratio = kabsch(s, p)
        if SIGMA2_FLOOR / SIGMA2_BAND < ratio < SIGMA2_FLOOR * SIGMA2_BAND:
            out["excluded"][k] = True
        if T is None:
            out["status"][k] = DEGENERATE
            continue
        E, bR, bt = bound(T, aux, A, md)
        out["T"][k], out["bR"][k], out["bt"][k], out["E"][k] = T, bR, bt, E
        d = dist64(T, s, p)
        if (np.abs(d - md) <= E).any():
            out["excluded"][k] = True
        if (d > md).any():
            out["status"][k] = FAR
            continue
        out["status"][k] = OK
        d = dist64(T, s_all, p_all)
        out["certain_mask"][k] = d < md - E
        out["uncertain_mask"][k] = np.abs(d - md) <= E
        out["certain"][k], out["uncertain"][k] = out["certain_mask"][k].sum(), out["uncertain_mask"][k].sum()
    return out


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def rigid(rng, angle=None, shift=0.5):
    """A random rigid motion: a rotation about a random axis (by ``angle``, default up to pi) and a translation up to ``shift``."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(0.3, np.pi) if angle is None else angle
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    T[:3, 3] = rng.uniform(-shift, shift, size=3)
    return T


def scene(seed, true_share=0.6, c=200, targets=400, noise=1e-3):
    """400 target points in the unit cube; the source: the inverse of a planted motion T0 applied to a subset, plus noise, so that
    T0 maps source onto target; c pairs, the first share true (source row i <-> its target row), the rest random rows, shuffled."""
    rng = np.random.default_rng(seed)
    P = rng.random((targets, 3)).astype(np.float32)
    T0 = rigid(rng)
    rows = rng.permutation(targets)[:c]
    Sd = (P[rows].astype(np.float64) - T0[:3, 3]) @ T0[:3, :3] + rng.normal(scale=noise, size=(c, 3))  # R^T (p - t)
    S = Sd.astype(np.float32)
    pairs = np.stack([np.arange(c), rows], axis=1)
    wrong = np.arange(c) >= int(round(true_share * c))
    pairs[wrong, 1] = rng.integers(0, targets, size=int(wrong.sum()))
    pairs = pairs[rng.permutation(c)].astype(np.int32)
    return dict(S=S, P=P, pairs=pairs, T0=T0, noise=noise)


def collinear_scene():
    """Three pairs whose points lie on one line, exactly: every sample that draws them all is degenerate."""
    P = np.float32([[0.25, 0.5, 0.75], [0.5, 0.5, 0.75], [1.0, 0.5, 0.75], [0.1, 0.9, 0.3]])
    S = np.float32([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.75, 0.0, 0.0]])
    return dict(S=S, P=P, pairs=np.int32([[0, 0], [1, 1], [2, 2]]))


MAX_DIST = 0.02
SCENE_SEEDS = {3: 11, 4: 12}  # by ransac_n
TRIAL_SEED = 7
TRIALS = 512
_cache = {}


def scene_trials(n, sim=0.9):
    """The scene of ransac_n = n and the spec's view of its TRIALS trials at TRIAL_SEED, computed once."""
    key = (n, sim)
    if key not in _cache:
        sc = scene(SCENE_SEEDS[n])
        _cache[key] = (sc, run_trials(sc["S"], sc["P"], sc["pairs"], n, MAX_DIST, sim, TRIAL_SEED, np.arange(TRIALS)))
    return _cache[key]


VIEW_NOISE = 1e-3
VIEW_MAX_DIST = 10 * VIEW_NOISE
VIEW_GAP = 3 * VIEW_MAX_DIST


def two_views(seed=5, count=2000, overlap=0.7):
    """Two views of ONE sampled surface, a bumpy height field (no plane: an FPFH must tell its points apart): the surface is
    sampled once, ``count`` points per unit of x over x in [0, 2 - overlap]; the target is the points with x < 1, the source those
    with x >= 1 - overlap, moved by the inverse of T0 and given sensor noise of VIEW_NOISE per coordinate.  So ``overlap`` of each
    view's extent is shared, and a shared point and its twin differ by the noise alone.
    VIEW_MAX_DIST is ten times the noise: the norm of the noise exceeds it with a probability below e^-40, so under the planted
    motion, and under any motion within a few noise scales of it, every shared point is an inlier -- the count a refinement can
    only keep or raise -- while it stays below half the points' mean spacing 1 / (2 sqrt(count)) = 0.011, so that a partner is the
    twin or a point next to it.  The source's own part starts VIEW_GAP = 3 VIEW_MAX_DIST beyond the target's edge (the points of
    the strip between are in neither view), so no motion within VIEW_MAX_DIST of the planted one gives a point of it a partner:
    the shared points are then the most inliers any such motion can have, and a refinement that converges reaches that count."""
    rng = np.random.default_rng(seed)
    length = 2.0 - overlap
    total = int(round(count * length))
    x, y = length * rng.random(total), rng.random(total)
    z = 0.15 * np.sin(7.0 * x) * np.cos(5.0 * y) + 0.1 * np.sin(13.0 * x * y / length) + 0.08 * np.cos(11.0 * y) + 0.05 * np.sin(23.0 * x + 3.0 * y)
    W = np.stack([x, y, z], axis=1)
    P = W[x < 1.0]
    Q = W[(x >= 1.0 - overlap) & ~((x >= 1.0) & (x < 1.0 + VIEW_GAP))]  # the source in the target's frame, before the noise
    T0 = rigid(rng, shift=0.3)
    S = (Q - T0[:3, 3]) @ T0[:3, :3] + rng.normal(scale=VIEW_NOISE, size=Q.shape)
    # where each view was seen from, in its own frame: five units above its middle
    view_p, view_q = np.array([0.5, 0.5, 5.0]), np.array([1.5 - overlap, 0.5, 5.0])
    return dict(P=P.astype(np.float32), S=S.astype(np.float32), T0=T0, Q=Q, view_p=view_p, view_s=(view_q - T0[:3, 3]) @ T0[:3, :3],
                shared=int((Q[:, 0] < 1.0).sum()))
