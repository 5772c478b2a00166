"""TrueKNN.icp (tknnIcp, include/owlknn_icp.h) against tests/icp_spec.py: one step from a given init -- the pairs exactly, the
evaluation and the transform within the derived bounds -- over the sizes at which the kernels take another path; the whole loop on a
surface; and two runs bit for bit."""
import contextlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_spec as spec  # noqa: E402

pytestmark = pytest.mark.gpu

METHODS = ("point_to_point", "point_to_plane")


def rot(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def cloud(seed, n, m, shift=0.0, dup=0.0):
    """A uniform target in the unit cube (+ shift), random unit normals of which a few are not finite, a source of m target points
    with noise, and an init a little off the identity about the cloud's middle."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    if dup:
        k = max(1, int(dup * n))
        P[rng.choice(n, k, replace=False)] = P[rng.choice(n, k)]
    P = (P + np.float32(shift)).astype(np.float32)
    nrm = unit(rng.normal(size=(n, 3)))
    if n >= 40:
        nrm[rng.choice(n, max(1, n // 50), replace=False), rng.integers(0, 3)] = np.nan
    S = (P[rng.integers(0, n, size=m)] + rng.normal(size=(m, 3)).astype(np.float32) * np.float32(0.004)).astype(np.float32)
    R = rot([1, 2, 3], 0.4)
    mid = np.full(3, 0.5 + shift)
    T0 = spec.rigid(R, mid - R @ mid + [0.003, -0.002, 0.001])
    return P, nrm, S, T0


# name: (seed, n, m, max_dist, what else)
CASES = {
    "uniform": dict(seed=1, n=5000, m=3000, max_dist=0.05),
    "n40": dict(seed=2, n=40, m=300, max_dist=0.3),       # three leaf blocks under a one-level pyramid
    "n1": dict(seed=3, n=1, m=70, max_dist=0.5),
    "m1": dict(seed=4, n=5000, m=1, max_dist=0.1),
    "m65": dict(seed=5, n=5000, m=65, max_dist=0.1),      # a partial wave of the moment kernel
    "m257": dict(seed=6, n=5000, m=257, max_dist=0.1),    # a partial workgroup
    "duplicates": dict(seed=7, n=5000, m=3000, max_dist=0.05, dup=0.05),
    "nan_source": dict(seed=8, n=5000, m=1000, max_dist=0.05, nan=True),
    "all_far": dict(seed=9, n=5000, m=500, max_dist=0.05, far=True),
    "shifted": dict(seed=10, n=5000, m=3000, max_dist=0.05, shift=1000.0),
    "whole_set": dict(seed=11, n=5000, m=3000, max_dist=10.0),  # the clipped seed bound
}


def make(name):
    c = CASES[name]
    P, nrm, S, T0 = cloud(c["seed"], c["n"], c["m"], shift=c.get("shift", 0.0), dup=c.get("dup", 0.0))
    if c.get("nan"):
        S[::7, 1] = np.nan
        S[3, :] = np.nan
    if c.get("far"):
        S = (S + np.float32(5)).astype(np.float32)
    return P, nrm, S, T0, c["max_dist"]


@contextlib.contextmanager
def fallback(on):
    before = os.environ.pop("TKNN_ICP_FORCE_FALLBACK", None)
    if on:
        os.environ["TKNN_ICP_FORCE_FALLBACK"] = "1"
    try:
        yield
    finally:
        os.environ.pop("TKNN_ICP_FORCE_FALLBACK", None)
        if before is not None:
            os.environ["TKNN_ICP_FORCE_FALLBACK"] = before


def one_step(name, method, robust, forced=False):
    from owlraytracing_amd.trueknn import TrueKNN

    P, nrm, S, T0, max_dist = make(name)
    m = len(S)
    scale = None if robust is None else (0.006 if method == "point_to_point" else 0.003)
    kw = dict(init=T0, method=method, target_normals=nrm if method == "point_to_plane" else None, robust=robust, robust_scale=scale,
              want_correspondences=True, want_aligned=True)
    eng = TrueKNN(device=0)
    try:
        eng.build(P)
        with fallback(forced):
            r0 = eng.icp(S, max_dist, max_iterations=0, **kw)
            r1 = eng.icp(S, max_dist, max_iterations=1, **kw)
    finally:
        eng.close()
    # ---- the evaluation at init: the pairs and their distances exactly ----
    w0 = spec.icp(P, S, max_dist, init=T0, method=method, normals=nrm, robust=robust, scale=scale, max_iterations=0)
    assert np.array_equal(r0["transform"].numpy(), T0) and (r0["iterations"], r0["searches"], r0["converged"], r0["degenerate"]) == (0, 1, 0, 0)
    assert np.array_equal(r0["aligned"].cpu().numpy().view(np.int32), w0["aligned"].view(np.int32)), "s' = Tf s, bit for bit"
    assert np.array_equal(r0["corr"].cpu().numpy(), w0["corr"]), "the pairs"
    assert np.array_equal(r0["corr_dist"].cpu().numpy().view(np.int32), w0["corr_dist"].view(np.int32)), "their fp32 distances"
    for field in ("correspondences", "fitness", "skipped_pairs"):
        assert r0[field] == w0[field], field
    print("%s %s %s: N %d skipped %d rmse %.9g (spec %.9g)" % (name, method, robust, r0["correspondences"], r0["skipped_pairs"], r0["inlier_rmse"], w0["inlier_rmse"]))
    assert abs(r0["inlier_rmse"] - w0["inlier_rmse"]) <= 64 * m * spec.EPS * w0["inlier_rmse"]
    assert (r0["lane_rows"] == m if forced else r0["lane_rows"] <= m) and (r0["point_tests"] > 0 or r0["correspondences"] == 0)
    # ---- one step ----
    w1 = spec.icp(P, S, max_dist, init=T0, method=method, normals=nrm, robust=robust, scale=scale, max_iterations=1)
    assert (r1["iterations"], r1["degenerate"], r1["converged"]) == (w1["iterations"], w1["degenerate"], w1["converged"])
    T = r1["transform"].numpy()
    if w1["degenerate"]:
        assert np.array_equal(T, T0) and r1["searches"] == 1
    else:
        bR, bt = w1["history"][0]["bound"]
        eR, et = np.abs(T[:3, :3] - w1["transform"][:3, :3]).max(), np.abs(T[:3, 3] - w1["transform"][:3, 3]).max()
        print("    step: rotation off by %.3g (bound %.3g), translation by %.3g (bound %.3g)" % (eR, bR, et, bt))
        assert eR <= bR and et <= bt and np.array_equal(T[3], [0, 0, 0, 1]) and r1["searches"] == 2
        assert not np.array_equal(T, T0)
    # the last search, at the device's own T: the same pairs as the spec finds there
    X = spec.apply(T, S)
    corr, dist = spec.correspond(P, X, max_dist)
    assert np.array_equal(r1["aligned"].cpu().numpy().view(np.int32), X.view(np.int32))
    assert np.array_equal(r1["corr"].cpu().numpy(), corr) and np.array_equal(r1["corr_dist"].cpu().numpy().view(np.int32), dist.view(np.int32))
    mom = spec.moments(P, X, corr, spec.centre(P), method, nrm, robust, scale)
    assert r1["correspondences"] == mom[spec.PAIRS] == (corr >= 0).sum() and r1["fitness"] == mom[spec.PAIRS] / m and r1["skipped_pairs"] == mom[spec.SKIPPED]
    rmse = np.sqrt(mom[spec.SUM_D2] / mom[spec.PAIRS]) if mom[spec.PAIRS] else 0.0
    assert abs(r1["inlier_rmse"] - rmse) <= 64 * m * spec.EPS * rmse
    return r0, r1, w0, w1


@pytest.mark.parametrize("robust", [None, "huber", "tukey"])
@pytest.mark.parametrize("method", METHODS)
def test_one_step_uniform(method, robust):
    r0, r1, w0, w1 = one_step("uniform", method, robust)
    assert r1["iterations"] == 1 and 0.9 < r0["fitness"] <= 1.0
    if method == "point_to_plane":
        assert r0["skipped_pairs"] > 0, "the case has normals that are not finite among the partners"
    if robust is None:
        assert r1["inlier_rmse"] < r0["inlier_rmse"] or method == "point_to_plane"


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", [n for n in CASES if n != "uniform"])
def test_one_step_edges(name, method):
    r0, r1, w0, w1 = one_step(name, method, None)
    if name in ("n1", "m1", "all_far"):
        assert r1["degenerate"] == 1 and r1["iterations"] == 0
    else:
        assert r1["iterations"] == 1
    if name == "all_far":
        assert r0["correspondences"] == 0 and r0["fitness"] == 0 and r0["inlier_rmse"] == 0 and (r0["corr"] == -1).all()
    if name == "nan_source":
        corr = r0["corr"].cpu().numpy()
        assert (corr[::7] == -1).all() and corr[3] == -1 and (corr >= 0).any()
    if name == "duplicates":
        P = make(name)[0]
        hit = r0["corr"].cpu().numpy()
        hit = hit[hit >= 0]
        first = {}
        for i, p in enumerate(map(tuple, P)):
            first.setdefault(p, i)
        twins = sum(1 for p, i in zip(map(tuple, P), range(len(P))) if first[p] != i)
        assert twins >= 200 and all(first[tuple(P[i])] == i for i in hit), "a duplicated point is named by its smaller row"
        assert sum(1 for i in set(hit.tolist()) if (P == P[i]).all(axis=1).sum() > 1) > 20, "the case has partners with a twin"
    if name == "whole_set":
        assert r0["fitness"] == 1.0
        # the seed bound is clipped, not max_dist walked: the work is that of the small radius
        assert r0["point_tests"] < 64 * 16 * len(make(name)[2])


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["uniform", "n40", "nan_source"])
def test_forced_fallback_gives_identical_outputs(name, method):
    a0, a1, _, _ = one_step(name, method, None)
    b0, b1, _, _ = one_step(name, method, None, forced=True)
    for a, b in ((a0, b0), (a1, b1)):
        for field in ("corr", "corr_dist", "aligned"):
            assert np.array_equal(a[field].cpu().numpy().view(np.int32), b[field].cpu().numpy().view(np.int32)), field
        assert np.array_equal(a["transform"].numpy().view(np.int64), b["transform"].numpy().view(np.int64))
        for field in ("fitness", "inlier_rmse", "correspondences", "skipped_pairs", "iterations", "converged", "degenerate"):
            assert a[field] == b[field], field


# ---- the whole loop --------------------------------------------------------------------------------------------------------------------
LOOP_SEED = {"point_to_point": 0, "point_to_plane": 0}  # (any: the two methods need not share an input)
LOOP_MAX_DIST = 0.5
_loop = {}


def loop_case(method, seed=None):
    """A saddle z = 0.3 (x^2 - y^2) over [-1, 1]^2 with noise, 4000 points, its normals; the source: 2500 of its points moved by
    the inverse of a known motion (10 degrees, 5 % of the extent), so that the motion is what the loop must find."""
    rng = np.random.default_rng(1000 + (LOOP_SEED[method] if seed is None else seed))
    xy = rng.uniform(-1, 1, size=(4000, 2))
    z = 0.3 * (xy[:, 0] ** 2 - xy[:, 1] ** 2) + rng.normal(size=4000) * 0.002
    P = np.column_stack([xy, z]).astype(np.float32)
    nrm = unit(np.column_stack([-0.6 * xy[:, 0], 0.6 * xy[:, 1], np.ones(4000)]))
    R, t = rot([0.3, -0.5, 1.0], 10.0), np.array([0.06, -0.05, 0.04])  # |t| = 0.088: 5 % of the extent's 2 on two axes
    sub = rng.choice(4000, 2500, replace=False)
    S = ((P[sub].astype(np.float64) - t) @ R).astype(np.float32)  # p = R s + t
    return P, nrm, S, spec.rigid(R, t)


def loop_spec(method):
    if method not in _loop:
        P, nrm, S, motion = loop_case(method)
        w = spec.icp(P, S, LOOP_MAX_DIST, method=method, normals=nrm, max_iterations=30, check_gap=True)
        _loop[method] = (P, nrm, S, motion, w)
    return _loop[method]


@pytest.mark.parametrize("method", METHODS)
def test_whole_loop(method):
    from owlraytracing_amd.trueknn import TrueKNN

    P, nrm, S, motion, w = loop_spec(method)
    # The smallest relative gap between a source point's nearest and second-nearest target point, per search.  Over 2 500 points
    # and up to 31 searches it lies between 1e-6 and 6e-5 for every seed tried (35 for point-to-plane, 7 for point-to-point), so a precondition of 1e-4 on
    # it cannot be met; the pairs are demanded equal at every search without one, and a failure names the gap of that search.
    gaps = [h["min_gap"] for h in w["history"]]
    kw = dict(method=method, target_normals=nrm if method == "point_to_plane" else None)
    eng = TrueKNN(device=0)
    try:
        eng.build(P)
        r = eng.icp(S, LOOP_MAX_DIST, max_iterations=30, want_correspondences=True, **kw)
        # search i of the loop is the last search of the loop cut after i steps
        for i, h in enumerate(w["history"]):
            ri = eng.icp(S, LOOP_MAX_DIST, max_iterations=i, want_correspondences=True, **kw)
            assert np.array_equal(ri["corr"].cpu().numpy(), h["corr"]), "the pairs of search %d (smallest relative gap there: %.3g)" % (i, gaps[i])
            assert ri["iterations"] == i and np.array_equal(ri["corr"].cpu().numpy(), spec.correspond(P, spec.apply(ri["transform"].numpy(), S), LOOP_MAX_DIST)[0])
    finally:
        eng.close()
    assert (r["iterations"], r["converged"], r["degenerate"]) == (w["iterations"], w["converged"], w["degenerate"])
    assert r["searches"] == len(w["history"]) and r["iterations"] > 3
    T = r["transform"].numpy()
    bR = sum(h["bound"][0] for h in w["history"] if "bound" in h)
    bt = sum(h["bound"][1] for h in w["history"] if "bound" in h)
    eR, et = np.abs(T[:3, :3] - w["transform"][:3, :3]).max(), np.abs(T[:3, 3] - w["transform"][:3, 3]).max()
    print("%s: %d iterations, converged %d; against the spec: rotation off by %.3g (bound %.3g), translation by %.3g (bound %.3g)"
          % (method, r["iterations"], r["converged"], eR, bR, et, bt))
    assert eR <= bR and et <= bt
    # the motion itself: as close as the spec gets on this input, times 4
    own = np.abs(w["transform"] - motion).max()
    got = np.abs(T - motion).max()
    print("    against the motion: %.3g (the spec: %.3g); fitness %.6g rmse %.6g" % (got, own, r["fitness"], r["inlier_rmse"]))
    assert got <= 4 * own and r["fitness"] == w["fitness"]
    if method == "point_to_plane":  # (point-to-point slides along a smooth surface: 30 steps leave it some 3e-2 away)
        assert own < 1e-6 and r["converged"] == 1, "the loop found the motion"


@pytest.mark.parametrize("method", METHODS)
def test_two_runs_bit_for_bit(method):
    from owlraytracing_amd.trueknn import TrueKNN

    P, nrm, S, motion = loop_case(method)
    kw = dict(method=method, target_normals=nrm if method == "point_to_plane" else None, robust="huber", robust_scale=0.05, max_iterations=6)
    runs = []
    for _ in range(2):
        eng = TrueKNN(device=0)
        try:
            eng.build(P)
            runs.append(eng.icp(S, LOOP_MAX_DIST, **kw))
            runs.append(eng.icp(S, LOOP_MAX_DIST, **kw))
        finally:
            eng.close()
    for r in runs[1:]:
        assert np.array_equal(r["transform"].numpy().view(np.int64), runs[0]["transform"].numpy().view(np.int64))
        assert r["inlier_rmse"] == runs[0]["inlier_rmse"] and r["fitness"] == runs[0]["fitness"] and r["iterations"] == 6


def test_the_one_shot_and_the_evaluation():
    import owlraytracing_amd

    P, nrm, S, T0, max_dist = make("uniform")
    r = owlraytracing_amd.icp(P, S, max_dist, init=T0, max_iterations=2)
    assert r["transform"].shape == (4, 4) and r["iterations"] == 2 and r["build_info"]
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    try:
        eng.build(P)
        e = eng.evaluate_registration(S, max_dist, init=T0)
        w = spec.icp(P, S, max_dist, init=T0, max_iterations=0)
        assert e["fitness"] == w["fitness"] and e["correspondences"] == w["correspondences"] and e["iterations"] == 0
        with pytest.raises(ValueError):
            eng.icp(S, max_dist, method="plane")
        with pytest.raises(ValueError):
            eng.icp(S, max_dist, method="point_to_plane")
        with pytest.raises(ValueError):
            eng.icp(S, max_dist, robust="huber")
        with pytest.raises(ValueError):
            eng.icp(S, max_dist, init=np.eye(3))
        with pytest.raises(ValueError):
            eng.icp(S.astype(np.float64)[:, :1], max_dist)
    finally:
        eng.close()
