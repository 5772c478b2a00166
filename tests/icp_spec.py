"""What TrueKNN.icp (tknnIcp, include/owlknn_icp.h) must give, restated in numpy: the literal fp32 transform and brute-force
correspondences, the moments, both solves and the loop in float64 with numpy's SVD and solve, and the error bounds the device's and
the host solver's results are held to.  No tests here."""
import numpy as np

EPS = np.finfo(np.float64).eps
MOMENTS = 32  # a moment row (owlraytracing_amd/csrc/icp_solve.h)
PAIRS, SUM_D2, SKIPPED, POSITIVE, SYSTEM, PLANE_RHS = 0, 1, 2, 3, 4, 25
SIGMA2_FLOOR = 2.0 ** -40  # point-to-point: sigma2 <= this times sigma1 is degenerate
PIVOT_FLOOR = 2.0 ** -40  # point-to-plane: a Cholesky pivot <= this times its diagonal entry is degenerate


def apply(T, S):
    """s' = Tf s: the top three rows of T rounded to fp32, ((Tf0*x + Tf1*y) + Tf2*z) + Tf3, every operation fp32."""
    Tf = np.asarray(T, np.float64)[:3].astype(np.float32)
    S = np.asarray(S, np.float32)
    x, y, z = S[:, 0], S[:, 1], S[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((Tf[i, 0] * x + Tf[i, 1] * y) + Tf[i, 2] * z) + Tf[i, 3] for i in range(3)], axis=1).astype(np.float32)


def correspond(P, X, max_dist, want_second=False, chunk=512):
    """c(j): the row of the nearest point of P within max_dist of X[j] in the literal fp32 distance, ties to the smaller row, -1
    for none; its distance (+inf for none); with ``want_second`` also the nearest and second-nearest distances whatever max_dist."""
    P, X = np.asarray(P, np.float32), np.asarray(X, np.float32)
    m = len(X)
    corr, dist = np.full(m, -1, np.int32), np.full(m, np.inf, np.float32)
    first, second = np.full(m, np.inf, np.float32), np.full(m, np.inf, np.float32)
    r = np.float32(max_dist)
    with np.errstate(all="ignore"):
        for lo in range(0, m, chunk):
            q = X[lo:lo + chunk]
            d = [P[None, :, a] - q[:, None, a] for a in range(3)]
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            dd = np.sqrt(d2)
            dd = np.where(np.isnan(dd), np.float32(np.inf), dd)
            best = np.argmin(dd, axis=1)  # the first minimum: the smaller row
            bd = dd[np.arange(len(q)), best]
            ok = bd <= r
            corr[lo:lo + chunk] = np.where(ok, best, -1)
            dist[lo:lo + chunk] = np.where(ok, bd, np.float32(np.inf))
            if want_second:
                first[lo:lo + chunk] = bd
                if P.shape[0] > 1:
                    second[lo:lo + chunk] = np.partition(dd, 1, axis=1)[:, 1]
    return (corr, dist, first, second) if want_second else (corr, dist)


def centre(P):
    """The centre of the scene box of the points without a NaN, from its fp32 corners."""
    P = np.asarray(P, np.float32)
    P = P[~np.isnan(P).any(axis=1)]
    return 0.5 * (P.min(axis=0).astype(np.float64) + P.max(axis=0).astype(np.float64))


def weights(robust, e, c):
    e = np.asarray(e, np.float64)
    if robust in (None, "l2"):
        return np.ones_like(e)
    c = float(np.float32(c))
    with np.errstate(all="ignore"):
        if robust == "huber":
            return np.where(e <= c, 1.0, c / e)
        if robust == "tukey":
            return np.where(e <= c, (1.0 - (e / c) ** 2) ** 2, 0.0)
    raise ValueError(robust)


def moments(P, X, corr, c, method="point_to_point", normals=None, robust=None, scale=None):
    """The moment row of the pairs (X[j], P[corr[j]]), coordinates relative to ``c``."""
    P, X = np.asarray(P, np.float32), np.asarray(X, np.float32)
    mom = np.zeros(MOMENTS)
    j = np.nonzero(corr >= 0)[0]
    s, p = X[j].astype(np.float64), P[corr[j]].astype(np.float64)
    d = s - p
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    mom[PAIRS], mom[SUM_D2] = len(j), d2.sum()
    a, b = s - c, p - c
    if method == "point_to_point":
        w = weights(robust, np.sqrt(d2), scale)
        mom[POSITIVE] = (w > 0).sum()
        mom[4] = w.sum()
        mom[5:8] = (w[:, None] * a).sum(axis=0)
        mom[8:11] = (w[:, None] * b).sum(axis=0)
        mom[11:20] = np.einsum("j,ji,jt->it", w, a, b).reshape(9)
        return mom
    n = np.asarray(normals, np.float32)[corr[j]].astype(np.float64)
    good = np.isfinite(n).all(axis=1)
    mom[SKIPPED] = (~good).sum()
    a, d, n = a[good], d[good], n[good]
    r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    w = weights(robust, np.abs(r), scale)
    mom[POSITIVE] = (w > 0).sum()
    J = np.concatenate([np.cross(a, n), n], axis=1)
    A = np.einsum("j,ji,jt->it", w, J, J)
    mom[SYSTEM:SYSTEM + 21] = A[np.triu_indices(6)]
    mom[PLANE_RHS:PLANE_RHS + 6] = (w[:, None] * J * r[:, None]).sum(axis=0)
    return mom


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def solve_point(mom, c):
    """dT of the point-to-point step from a moment row, or None where it is degenerate; and what the bound needs:
    dict(H, sigma (sigma3 signed by det(V U^T)), mu_s, mu_p)."""
    W = mom[4]
    if not (mom[POSITIVE] >= 3 and W > 0 and np.isfinite(mom[:20]).all()):
        return None, None
    Sa, Sb, Sab = mom[5:8], mom[8:11], mom[11:20].reshape(3, 3)
    H = Sab - np.outer(Sa, Sb) / W
    U, S, Vt = np.linalg.svd(H)
    if not S[1] > SIGMA2_FLOOR * S[0]:
        return None, None
    V = Vt.T
    det = np.sign(np.linalg.det(V @ U.T))
    R = V @ np.diag([1.0, 1.0, det]) @ U.T
    mus, mup = c + Sa / W, c + Sb / W
    return rigid(R, mup - R @ mus), dict(H=H, sigma=np.array([S[0], S[1], det * S[2]]), mu_s=mus, mu_p=mup)


def plane_system(mom):
    """The 6 x 6 system of the sums, J = [(s' - c) x n, n]."""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = mom[SYSTEM:SYSTEM + 21]
    return A + np.triu(A, 1).T, mom[PLANE_RHS:PLANE_RHS + 6]


def euler(x):
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def solve_plane(mom, c):
    """dT of the point-to-plane step, or None where a Cholesky pivot is not above PIVOT_FLOOR times its diagonal entry or not
    finite; and dict(A, x)."""
    A, g = plane_system(mom)
    L = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j, j] - (L[j, :j] ** 2).sum()
            if not (d > PIVOT_FLOOR * A[j, j] and np.isfinite(d)):
                return None, None
            L[j, j] = np.sqrt(d)
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    x = np.linalg.solve(A, -g)
    if not np.isfinite(x).all():
        return None, None
    R = euler(x)
    return rigid(R, c - R @ c + x[3:]), dict(A=A, x=x, c=np.asarray(c, np.float64))


def point_bound(aux, factor=1.0):
    """(on the entries of dR, on the entries of dt): 64 eps |H|_F / (sigma2 + sigma3) -- the gap of Horn's matrix between its two
    largest eigenvalues is 2 (sigma2 + sigma3), sigma3 signed -- and dt = mu_p - dR mu_s carries dR's error times |mu_s|_1 plus
    the rounding of the centroids."""
    s = aux["sigma"]
    bR = 64 * EPS * np.linalg.norm(aux["H"]) / (s[1] + s[2]) * factor
    bt = bR * np.abs(aux["mu_s"]).sum() + 64 * EPS * factor * (np.abs(aux["mu_p"]).max() + np.abs(aux["mu_s"]).sum())
    return bR, bt


def plane_bound(aux, factor=1.0):
    """(on the entries of dR, on the entries of dt): 64 eps cond(J^T J) on x; an entry of Rz Ry Rx moves by at most 2 per unit of
    each of its three angles, and dt = c - dR c + t carries dR's error times |c|_1."""
    bx = 64 * EPS * np.linalg.cond(aux["A"]) * factor
    return 6 * bx, 6 * bx * np.abs(aux["c"]).sum() + bx + 64 * EPS * factor * np.abs(aux["c"]).max()


def compose_bound(bR, bt, T0):
    """What the bounds on dT allow on T = dT T0: (on the rotation entries, on the translation entries)."""
    return 3 * bR, 3 * bR * np.abs(T0[:3, 3]).max() + bt


def icp(P, S, max_dist, init=None, method="point_to_point", normals=None, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6,
        robust=None, scale=None, check_gap=None):
    """The loop of include/owlknn_icp.h.  dict(transform, fitness, inlier_rmse, correspondences, skipped_pairs, iterations,
    converged, degenerate, corr, corr_dist, aligned, history: per search dict(T, corr, bound (on T after the step: rotation,
    translation), min_gap (with ``check_gap``: the smallest relative gap between a point's nearest and second-nearest distance)))."""
    P, S = np.asarray(P, np.float32), np.asarray(S, np.float32)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    m = len(S)
    out = dict(transform=T, fitness=0.0, inlier_rmse=0.0, correspondences=0, skipped_pairs=0, iterations=0, converged=0, degenerate=0,
               corr=np.zeros(0, np.int32), corr_dist=np.zeros(0, np.float32), aligned=np.zeros((0, 3), np.float32), history=[])
    if m == 0:
        return out
    c = centre(P)
    prev = None
    while True:
        X = apply(T, S)
        h = dict(T=T.copy())
        if check_gap is not None:
            corr, dist, first, second = correspond(P, X, max_dist, want_second=True)
            with np.errstate(all="ignore"):
                gap = np.where(np.isfinite(first), (second - first) / np.maximum(second, np.float32(1e-30)), np.inf)
            h["min_gap"] = float(gap.min())
        else:
            corr, dist = correspond(P, X, max_dist)
        mom = moments(P, X, corr, c, method, normals, robust, scale)
        N = mom[PAIRS]
        out.update(transform=T, corr=corr, corr_dist=dist, aligned=X, correspondences=int(N), skipped_pairs=int(mom[SKIPPED]),
                   fitness=N / m, inlier_rmse=float(np.sqrt(mom[SUM_D2] / N)) if N > 0 else 0.0)
        h.update(corr=corr, fitness=out["fitness"], inlier_rmse=out["inlier_rmse"])
        out["history"].append(h)
        if prev is not None and abs(out["fitness"] - prev[0]) < rel_fitness and abs(out["inlier_rmse"] - prev[1]) < rel_rmse:
            out["converged"] = 1
            break
        if out["iterations"] == max_iterations:
            break
        dT, aux = (solve_plane if method == "point_to_plane" else solve_point)(mom, c)
        if dT is None:
            out["degenerate"] = 1
            break
        bR, bt = (plane_bound if method == "point_to_plane" else point_bound)(aux, factor=m)
        h["bound"] = compose_bound(bR, bt, T)
        T = dT @ T
        out["iterations"] += 1
        prev = (out["fitness"], out["inlier_rmse"])
    return out
