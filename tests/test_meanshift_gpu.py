"""TrueKNN.mean_shift_modes (tknnMeanShift, include/owlknn_meanshift.h), TrueKNN.mean_shift and bin_seeds against
tests/meanshift_spec.py: one step inside the derived bound through the team walk and through the lane kernel, for the three kernels,
on the smallest shapes at which each mechanism can go wrong; the loop as the iterated step, bit for bit; the blob set end to end."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import meanshift_spec as ms  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
FALLBACK, REORDER = "TKNN_MEANSHIFT_FORCE_FALLBACK", "TKNN_MEANSHIFT_REORDER"
R, H = F(0.08), F(0.03)  # the radius of the one-step cases and the Gauss bandwidth that goes with it
ARRAYS = ("modes", "counts", "wsum", "shift", "iterations", "status")


@pytest.fixture(scope="module")
def eng():
    from owlraytracing_amd.trueknn import TrueKNN

    e = TrueKNN(device=0)
    yield e
    e.close()


def call(eng, X, r, kernel, tol=0.0, max_iterations=1, h=H):
    """One call, its tensors as numpy."""
    res = eng.mean_shift_modes(float(h), seeds=X, kernel=kernel, radius=float(r), tol=float(tol), max_iterations=max_iterations)
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def bits(res):
    return {k: (res[k].view(np.uint32) if res[k].dtype == np.float32 else res[k]) for k in ARRAYS}


def same_bits(a, b, what):
    a, b = bits(a), bits(b)
    for k in ARRAYS:
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


def one_step(eng, monkeypatch, key, P, X, r=R, kernels=ms.KERNELS, own=False):
    """The built set's step from X (own: from its own points) through both kernels, held to the spec; the counts are radius_reduce's."""
    m = len(P) if own else len(X)
    seeds = np.ascontiguousarray(P if own else X, F)
    reduce_counts = eng.radius_reduce(float(r), queries=None if own else X, want_wsum=False)["counts"].cpu().numpy()
    for kernel in kernels:
        want = ms.want_step(key, P, seeds, r, kernel, H)
        for fallback in ("0", "1"):
            monkeypatch.setenv(FALLBACK, fallback)
            got = call(eng, None if own else X, r, kernel)
            ms.compare_step(got, want, kernel, r, H, X=seeds)
            assert np.array_equal(got["counts"], reduce_counts)
            info = got["info"]
            assert info["iterations"] == 1 and info["walks"] == m and info["fallback_items"] == (m if fallback == "1" else info["fallback_items"])
            assert info["converged"] + info["empty"] + info["running"] + info["invalid"] == m
            assert info["empty"] == (got["status"] == ms.EMPTY).sum() and info["invalid"] == (got["status"] == ms.INVALID).sum()
            assert info["running"] == (got["status"] == ms.RUNNING).sum() and info["solve_ms"] > 0 and info["walk_ms"] > 0


def seeds_with_edges(X):
    """X with a NaN seed, seeds 5 units away (no neighbours) and a seed that is far on one axis only."""
    X = X.copy()
    X[3] = [np.nan, 0.5, 0.5]
    X[11] = [0.5, 0.5, np.nan]
    X[17] = [5.5, 5.5, 5.5]
    X[23] = [-4.5, 0.5, 0.5]
    return X


def test_one_step_uniform(eng, monkeypatch):
    P, X = ms.uniform_case()
    X = seeds_with_edges(X)
    eng.build(P)
    want = ms.want_step("uniform", P, X, R, "flat", H)
    assert 8 < want["len"].mean() < 13 and (want["len"] == 0).sum() >= 4
    one_step(eng, monkeypatch, "uniform", P, X)


@pytest.mark.parametrize("m", (1, 65, 257))
def test_one_step_few_seeds(eng, monkeypatch, m):
    P, X = ms.uniform_case()
    eng.build(P)
    one_step(eng, monkeypatch, "uniform_m%d" % m, P, np.ascontiguousarray(seeds_with_edges(X)[:m]))


@pytest.mark.parametrize("n", (1, 40, 1025))
def test_one_step_small_trees_and_a_last_block_of_one_point(eng, monkeypatch, n):
    """n = 1 and 40: no box pyramid, every row is the lane kernel's; 1 025 points end in a leaf block of one point."""
    rng = np.random.default_rng(100 + n)
    P = rng.random((n, 3), dtype=F)
    X = (P[rng.integers(0, n, 70)] + (rng.random((70, 3), dtype=F) - F(0.5)) * F(0.05)).astype(F)
    X = np.concatenate([X, P[:1], F([[3, 3, 3], [np.nan, 0.5, 0.5]])]).astype(F)
    eng.build(P)
    r = F(0.3) if n <= 40 else F(0.12)
    one_step(eng, monkeypatch, "small%d" % n, P, X, r)
    one_step(eng, monkeypatch, "small_own%d" % n, P, None, r, kernels=("gauss",), own=True)


def test_one_step_duplicates_ids_and_batches(eng, monkeypatch):
    """5 % of the points are copies of others; a tree built with permuted ids and a batched tree answer as the plain one."""
    P, X = ms.uniform_case()
    P = P[:2000].copy()
    rng = np.random.default_rng(41)
    dup = rng.choice(2000, 100, replace=False)
    P[dup] = P[(dup + 7) % 2000]
    X = X[:400].copy()
    X[:50] = P[dup[:50]]  # seeds on the copies themselves
    r = F(0.12)
    eng.build(P)
    one_step(eng, monkeypatch, "dups", P, X, r)
    one_step(eng, monkeypatch, "dups_own", P, None, r, kernels=("flat",), own=True)
    eng.build(P, ids=rng.permutation(2000).astype(np.int32))
    one_step(eng, monkeypatch, "dups", P, X, r)
    one_step(eng, monkeypatch, "dups_own", P, None, r, kernels=("flat",), own=True)
    eng.build(P, batch=rng.integers(0, 3, 2000).astype(np.int32), num_batches=3)
    one_step(eng, monkeypatch, "dups", P, X, r)
    one_step(eng, monkeypatch, "dups_own", P, None, r, kernels=("flat",), own=True)


def test_one_step_on_a_cloud_at_1000(eng, monkeypatch):
    """The sums are over offsets: the bound is the same as at the origin, up to the rounding of x' itself."""
    P, X = ms.uniform_case()
    P, X = (P + F(1000)).astype(F), (X[:600] + F(1000)).astype(F)
    eng.build(P)
    want = ms.want_step("shifted", P, X, R, "flat", H)
    assert want["len"].mean() > 5
    one_step(eng, monkeypatch, "shifted", P, X)


def test_one_step_with_every_box_inside(eng, monkeypatch):
    """Radius 10 on 5 000 points: every box is inside the sphere, the range list streams the whole set for every seed."""
    P, X = ms.uniform_case()
    X = np.ascontiguousarray(X[:48])
    eng.build(P)
    want = ms.want_step("all", P, X, F(10), "flat", H)
    assert (want["len"] == len(P)).all()
    one_step(eng, monkeypatch, "all", P, X, F(10), kernels=("flat", "epanechnikov"))
    # Gauss at a bandwidth that leaves weight at that distance
    for fallback in ("0", "1"):
        monkeypatch.setenv(FALLBACK, fallback)
        got = call(eng, X, F(10), "gauss", h=F(0.5))
        ms.compare_step(got, ms.want_step("all_h", P, X, F(10), "gauss", F(0.5)), "gauss", F(10), F(0.5), X=X)


def test_nan_and_infinite_points_reach_no_sum(eng, monkeypatch):
    """The leak test: some points of P hold NaN, +inf or -inf in a coordinate.  They are nobody's neighbour: every result is finite
    and inside the bound of the spec, which never sees them."""
    rng = np.random.default_rng(51)
    P = rng.random((1025, 3), dtype=F)
    bad = rng.choice(1025, 45, replace=False)
    P[bad, rng.integers(0, 3, 45)] = np.array([np.nan, np.inf, -np.inf], F)[np.arange(45) % 3]
    X = rng.random((200, 3), dtype=F)
    r = F(0.15)
    eng.build(P)
    for kernel in ms.KERNELS:
        want = ms.want_step("leak", P, X, r, kernel, H)
        assert (want["len"] > 0).all() and np.isfinite(want["new"]).all()
        for fallback in ("0", "1"):
            monkeypatch.setenv(FALLBACK, fallback)
            got = call(eng, X, r, kernel)
            assert all(np.isfinite(got[k]).all() for k in ("modes", "wsum", "shift"))
            ms.compare_step(got, want, kernel, r, H, X=X)
            own = call(eng, None, r, kernel)
            assert (own["status"][bad] != ms.RUNNING).all() and (own["counts"][bad] == 0).all()
            assert (own["status"][np.isnan(P).any(axis=1)] == ms.INVALID).all()
            ok = np.isfinite(P).all(axis=1)
            assert np.isfinite(own["modes"][ok]).all() and (own["status"][ok] <= ms.CONVERGED).all() and (own["counts"][ok] > 0).all()


@pytest.mark.parametrize("n", (3, 2000))
def test_a_weight_sum_that_underflows_is_invalid_not_a_step(eng, monkeypatch, n):
    """Gauss at a bandwidth so small that every weight of a seed's neighbours is exactly 0: W = 0, the step is 0 / 0.  The header:
    INVALID, the position unchanged, the step does not count, d_shift holds the NaN; the count and W are the walk's.  Seeds that sit
    on a point have weight 1 there and converge."""
    # a lattice of spacing 0.1 (a row of three points; 10 x 10 x 20), the first seeds midway between two points: every neighbour is at
    # 0.05 or more, exp(-0.05^2 / (2 * 1e-6)) = exp(-1250) = 0 in fp32 as in float64
    g = np.arange(20, dtype=np.float64) * 0.1
    P = (np.stack(np.meshgrid(g[:10], g[:10], g, indexing="ij"), axis=-1).reshape(-1, 3) if n > 3 else np.stack([g[:3], 0 * g[:3], 0 * g[:3]], axis=1)).astype(F)
    assert len(P) == n
    X = np.concatenate([(P[:3] + F([0.05, 0, 0])).astype(F), P[:2]])
    h, r = F(1e-3), F(0.2)
    want = ms.loop(P, X, r, "gauss", h, tol=1e-6, max_iterations=4)
    assert want["status"].tolist() == [ms.INVALID] * 3 + [ms.CONVERGED] * 2 and (want["wsum"][:3] == 0).all() and (want["counts"][:3] > 0).all()
    eng.build(P)
    for fallback in ("0", "1"):
        monkeypatch.setenv(FALLBACK, fallback)
        got = call(eng, X, r, "gauss", tol=1e-6, max_iterations=4, h=h)
        assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["counts"], want["counts"])
        assert np.array_equal(got["modes"][:3].view(np.uint32), X[:3].view(np.uint32)) and np.isnan(got["shift"][:3]).all()
        assert (got["iterations"][:3] == 0).all() and (got["wsum"][:3] == 0).all()
        assert np.array_equal(got["iterations"][3:], want["iterations"][3:]) and np.allclose(got["modes"][3:], want["modes"][3:], atol=1e-6)
        assert got["info"]["invalid"] == 3 and got["info"]["converged"] == 2 and got["info"]["walks"] == want["walks"]


def chain(eng, P, X, r, kernel, h, tol, T):
    """T calls of one step each, driven from here: the active set from the returned status, the positions fed back."""
    m = len(P) if X is None else len(X)
    out = {"modes": (P if X is None else X).copy(), "counts": np.zeros(m, np.int32), "wsum": np.zeros(m, F), "shift": np.full(m, np.inf, F),
           "iterations": np.zeros(m, np.int32), "status": np.zeros(m, np.uint8)}
    active = np.arange(m)
    walks = passes = 0
    for t in range(T):
        if len(active) == 0:
            break
        first_own = X is None and t == 0
        got = call(eng, None if first_own else np.ascontiguousarray(out["modes"][active]), r, kernel, tol=tol, max_iterations=1, h=h)
        assert got["info"]["iterations"] == 1 and got["info"]["walks"] == len(active)
        walks += len(active)
        passes += 1
        stepped = got["iterations"] == 1
        for k in ("modes", "counts", "wsum", "status"):
            out[k][active] = got[k]
        out["shift"][active] = np.where(stepped | np.isnan(got["shift"]) | (t == 0), got["shift"], out["shift"][active])
        out["iterations"][active] += got["iterations"]
        active = active[got["status"] == ms.RUNNING]
    return out, walks, passes


@pytest.mark.parametrize("fallback", ("0", "1"))
@pytest.mark.parametrize("variant", ("external", "own", "reorder"))
@pytest.mark.parametrize("kernel", ("flat", "gauss"))
def test_the_loop_is_the_iterated_step_bit_for_bit(eng, monkeypatch, kernel, variant, fallback):
    """One call with max_iterations = T equals T chained calls of one step: a row's sums depend on the tree, the position and the
    kernel that made them (radius_walk.h: the team's traversal and its lanes' shares are functions of the tree, q and r), not on the
    list position, the pass or what else is in the list -- so also not on TKNN_MEANSHIFT_REORDER."""
    P, X = ms.uniform_case()
    T = 12
    bw = 0.08 if kernel == "flat" else 0.03
    r, tol = ms.default_radius(kernel, bw), F(1e-3 * bw)
    seeds = None if variant == "own" else X
    eng.build(P)
    monkeypatch.setenv(FALLBACK, fallback)
    want, walks, passes = chain(eng, P, seeds, r, kernel, bw, tol, T)
    if variant == "reorder":
        monkeypatch.setenv(REORDER, "3")
    got = call(eng, seeds, r, kernel, tol=tol, max_iterations=T, h=bw)
    same_bits(got, want, "%s %s" % (kernel, variant))
    info = got["info"]
    assert info["walks"] == walks and info["iterations"] == passes == T
    assert fallback == "0" or info["fallback_items"] == walks
    m = len(want["status"])
    running, stopped = (got["status"] == ms.RUNNING).sum(), (got["iterations"] < T).sum()
    assert running > 0 and stopped > 0 and walks < m * T, "some seeds still move after T steps and others stopped early"
    assert info["running"] == running and info["converged"] == (got["status"] == ms.CONVERGED).sum()
    assert (got["iterations"][got["status"] == ms.RUNNING] == T).all()
    assert info["compact_ms"] > 0 and (info["order_ms"] > 0 or variant == "own")


def test_two_runs_bit_for_bit(eng, monkeypatch):
    P, X = ms.uniform_case()
    eng.build(P)
    for kernel, bw in (("flat", 0.08), ("gauss", 0.03), ("epanechnikov", 0.1)):
        for fallback in ("0", "1"):
            monkeypatch.setenv(FALLBACK, fallback)
            a = call(eng, X, ms.default_radius(kernel, bw), kernel, tol=1e-3 * bw, max_iterations=6, h=bw)
            b = call(eng, X, ms.default_radius(kernel, bw), kernel, tol=1e-3 * bw, max_iterations=6, h=bw)
            same_bits(a, b, kernel)
            assert a["info"]["walks"] == b["info"]["walks"]


@pytest.mark.parametrize("kernel", ("flat", "gauss"))
def test_blobs_end_to_end(eng, kernel):
    import owlraytracing_amd
    from owlraytracing_amd.trueknn import mean_shift as one_shot

    P, comp = ms.blobs()
    means = ms.blob_means()
    bw = ms.BLOB_KERNELS[kernel]["bandwidth"]
    eng.build(P)
    res = eng.mean_shift(bw, kernel=kernel, points=P)
    got = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}
    assert (got["status"] == ms.CONVERGED).all() and got["info"]["converged"] == len(P)
    assert got["info"]["walks"] < len(P) * got["info"]["iterations"], "the active set shrank"
    assert len(got["centers"]) == 4
    far = np.linalg.norm(got["centers"].astype(np.float64)[:, None] - means[None], axis=2).min(axis=1)
    assert (far <= 0.05 * bw).all()
    assert got["labels"].dtype == np.int64 and ms.same_partition(got["labels"], comp)
    # the merge and the labels are the spec's, applied to the device's own modes and scores, exactly
    scores = got["counts"] if kernel == "flat" else got["wsum"]
    want = ms.merge_and_label(P, got["modes"], scores, got["status"], got["counts"], bw)
    assert np.array_equal(got["centers"].view(np.uint32), want["centers"].view(np.uint32)) and np.array_equal(got["labels"], want["labels"])
    assert np.array_equal(got["scores"].view(np.uint32), want["scores"].view(np.uint32))
    if kernel == "flat":
        for helper in (one_shot, owlraytracing_amd.mean_shift):
            again = helper(P, bw)
            assert np.array_equal(again["centers"], got["centers"]) and np.array_equal(again["labels"], got["labels"])
        # two outliers, alone within the bandwidth: lone seeds are no candidates at min_count = 2, nobody is their centre
        Q = np.concatenate([P, F([[0.5, 0.5, 0.05], [0.05, 0.95, 0.05]])])
        eng.build(Q)
        res = eng.mean_shift(bw, points=Q, cluster_all=False, min_count=2)
        labels = res["labels"].cpu().numpy()
        assert len(res["centers"]) == 4 and (labels[-2:] == -1).all()
        want = ms.merge_and_label(Q, res["modes"].cpu().numpy(), res["counts"].cpu().numpy(), res["status"].cpu().numpy(), res["counts"].cpu().numpy(), bw,
                                  cluster_all=False, min_count=2)
        assert np.array_equal(labels, want["labels"]) and np.array_equal(res["centers"].cpu().numpy(), want["centers"])
        inside = labels[:-2] >= 0
        assert inside.mean() > 0.99 and ms.same_partition(labels[:-2][inside], comp[inside])
        # seeds from bins: the same four centres, up to where the trajectories end
        eng.build(P)
        binned = eng.mean_shift(bw, seeds=owlraytracing_amd.bin_seeds(P, bw), points=P)
        assert len(binned["centers"]) == 4 and ms.same_partition(binned["labels"].cpu().numpy(), comp)
        # a NaN point is labelled -1; no candidates: no centres, every label -1
        N = P.copy()
        N[7] = [np.nan, 0.2, 0.2]
        eng.build(N)
        res = eng.mean_shift(bw, points=N)
        assert res["labels"][7] == -1 and res["status"][7] == ms.INVALID and len(res["centers"]) == 4
        none = eng.mean_shift(bw, points=N, min_count=10 ** 6)
        assert tuple(none["centers"].shape) == (0, 3) and (none["labels"] == -1).all()
        with pytest.raises(ValueError):
            eng.mean_shift(bw)
        with pytest.raises(ValueError):
            eng.mean_shift_modes(bw, kernel="cubic_spline")


def test_bin_seeds(eng):
    import torch

    from owlraytracing_amd.trueknn import bin_seeds

    P, _ = ms.blobs()
    for pts, size, freq in ((P, 0.08, 1), (P, 0.08, 5), (((P - F(0.5)) * F(3)).astype(F), 0.25, 2), (P, 0.011, 1)):
        want = ms.bin_seeds(pts, size, freq)
        got = bin_seeds(pts, size, freq)
        assert got.is_cuda and got.dtype == torch.float32
        assert len(want) > 4 and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        shuffled = bin_seeds(torch.from_numpy(pts[np.random.default_rng(3).permutation(len(pts))].copy()).to(eng.device), size, freq)
        assert torch.equal(shuffled, got), "the seeds do not depend on the order of the points"
    with_nan = P.copy()
    with_nan[5] = [np.nan, 0, 0]
    assert np.array_equal(bin_seeds(with_nan, 0.08).cpu().numpy(), ms.bin_seeds(with_nan, 0.08))
