"""tknnIcp and the state that carries from one call to the next (tests/test_engine_state_gpu.py's rule, for the new call): the call
gives the same answer, bit for bit, on a fresh engine, after its scratch was poisoned and after unrelated calls on the same engine;
and those calls give what they gave without an icp before them."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BYTES = (0x00, 0xFF, 0x5A)
WORKSPACE = 4 << 20  # more than the calls here need: their layouts lie wholly inside the poisoned bytes
METHODS = ("point_to_point", "point_to_plane")


def case():
    rng = np.random.default_rng(12)
    xy = rng.uniform(-1, 1, size=(3000, 2))
    P = np.column_stack([xy, 0.3 * np.sin(2 * xy[:, 0]) * np.cos(2 * xy[:, 1])]).astype(np.float32)
    nrm = rng.normal(size=(3000, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    a = np.deg2rad(2.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    S = (P[rng.choice(3000, 1300, replace=False)].astype(np.float64) @ R.T + [0.01, -0.02, 0.015]).astype(np.float32)
    S[5, 0] = np.nan
    Q = rng.uniform(-1, 1, size=(500, 3)).astype(np.float32)
    return P, nrm, S, Q


@contextlib.contextmanager
def forced(on):
    before = os.environ.pop("TKNN_ICP_FORCE_FALLBACK", None)
    if on:
        os.environ["TKNN_ICP_FORCE_FALLBACK"] = "1"
    try:
        yield
    finally:
        os.environ.pop("TKNN_ICP_FORCE_FALLBACK", None)
        if before is not None:
            os.environ["TKNN_ICP_FORCE_FALLBACK"] = before


def engine(P):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(P)
    return eng


def icp(eng, method, nrm, S):
    r = eng.icp(S, 0.2, method=method, target_normals=nrm if method == "point_to_plane" else None, robust="huber", robust_scale=0.05,
                max_iterations=5, want_correspondences=True, want_aligned=True)
    return {"transform": r["transform"].numpy().view(np.int64), "corr": r["corr"].cpu().numpy(), "corr_dist": r["corr_dist"].cpu().numpy().view(np.int32),
            "aligned": r["aligned"].cpu().numpy().view(np.int32), "evaluation": np.float64([r["fitness"], r["inlier_rmse"]]).view(np.int64),
            "counts": np.int64([r["correspondences"], r["skipped_pairs"], r["iterations"], r["searches"], r["converged"], r["degenerate"]])}


def others(eng, Q):
    """An unrelated solve, knn and radius_reduce; their outputs as bits."""
    s = eng.solve(5, 0.05)
    k = eng.knn(Q, k=3)
    r = eng.radius_reduce(0.15, queries=Q, weight="epanechnikov")
    return {"solve.idx": s["idx"].cpu().numpy(), "solve.dist": s["dist"].cpu().numpy().view(np.int32), "knn.idx": k["idx"].cpu().numpy(),
            "knn.dist": k["dist"].cpu().numpy().view(np.int32), "reduce.wsum": r["wsum"].cpu().numpy().view(np.int32), "reduce.counts": r["counts"].cpu().numpy()}


def same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert np.array_equal(a[name], b[name]), "%s: %s differs" % (what, name)


@pytest.fixture(scope="module")
def fresh():
    P, nrm, S, Q = case()
    out = {}
    for method in METHODS:
        eng = engine(P)
        out[method] = icp(eng, method, nrm, S)
        eng.close()
        assert out[method]["counts"][2] >= 2 and out[method]["counts"][0] > 1000 and out[method]["corr"][5] == -1
    eng = engine(P)
    out["others"] = others(eng, Q)
    eng.close()
    return out


@pytest.mark.parametrize("fallback", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_poisoned_scratch(fresh, method, fallback):
    from owlraytracing_amd import _debug_lib

    P, nrm, S, Q = case()
    eng = engine(P)
    try:
        for byte in BYTES:
            assert _debug_lib.poison(eng, _debug_lib.POISON_ALL, byte, WORKSPACE) >= WORKSPACE
            with forced(fallback):
                same(icp(eng, method, nrm, S), fresh[method], "after poison 0x%02X" % byte)
    finally:
        eng.close()


@pytest.mark.parametrize("method", METHODS)
def test_between_other_calls(fresh, method):
    P, nrm, S, Q = case()
    eng = engine(P)
    try:
        same(others(eng, Q), fresh["others"], "the other calls on a fresh engine")
        same(icp(eng, method, nrm, S), fresh[method], "icp after solve, knn and radius_reduce")
        same(others(eng, Q), fresh["others"], "solve, knn and radius_reduce after an icp")
        same(icp(eng, method, nrm, S), fresh[method], "icp again")
        same(icp(eng, METHODS[1 - METHODS.index(method)], nrm, S), fresh[METHODS[1 - METHODS.index(method)]], "the other method after this one")
    finally:
        eng.close()
