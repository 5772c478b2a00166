"""tknnFeatureMatch and tknnRansac and the state that carries from one call to the next (tests/test_engine_state_gpu.py's rule, for the
new calls): both answer on an engine that has no tree; on an engine with a tree they give the same bits before and after other
calls, after the scratch was poisoned and after calls with a larger or smaller workspace; and the tree answers ``knn`` afterwards as
it did before."""
import numpy as np
import pytest

import global_spec as gs

pytestmark = pytest.mark.gpu

BYTES = (0x00, 0xFF, 0x5A)
WORKSPACE = 4 << 20  # more than the calls here need: their layouts lie wholly inside the poisoned bytes


def cases():
    rng = np.random.default_rng(9)
    return gs.fpfh_like(rng, 300), gs.fpfh_like(rng, 410), gs.scene_trials(3)[0]


def both(eng):
    """The two calls' outputs as bits, the times left out."""
    A, B, sc = cases()
    m = eng.match_features(A, B)
    r = eng.ransac(sc["S"], sc["P"], sc["pairs"], gs.MAX_DIST, confidence=1.0, max_trials=700, seed=gs.TRIAL_SEED, want_mask=True, want_trials=True)
    out = {"match." + k: m[k].cpu().numpy().view(np.int32) for k in ("best", "best_d2", "second_d2", "pairs")}
    out.update({"ransac." + k: r[k].cpu().numpy() for k in ("mask", "trial_status", "trial_inliers", "transform")})
    out["ransac.info"] = np.float64([r["best_trial"], r["inliers"], r["fitness"], r["inlier_rmse"], r["trials_run"], r["refits_kept"]] + list(r["status_counts"].values()))
    return out


def others(eng, Q):
    s = eng.solve(5, 0.05)
    k = eng.knn(Q, k=3)
    return {"solve.idx": s["idx"].cpu().numpy(), "solve.dist": s["dist"].cpu().numpy().view(np.int32), "knn.idx": k["idx"].cpu().numpy(),
            "knn.dist": k["dist"].cpu().numpy().view(np.int32)}


def same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert np.array_equal(a[name], b[name]), "%s: %s differs" % (what, name)


@pytest.fixture(scope="module")
def fresh():
    from owlraytracing_amd.trueknn import TrueKNN

    rng = np.random.default_rng(3)
    P, Q = rng.random((5000, 3), dtype=np.float32), rng.random((300, 3), dtype=np.float32)
    eng = TrueKNN(device=0)  # no tree
    out = {"calls": both(eng), "P": P, "Q": Q}
    assert eng.n == 0
    eng.close()
    eng = TrueKNN(device=0)
    eng.build(P)
    out["others"] = others(eng, Q)
    eng.close()
    A, B, sc = cases()
    best, b1, b2 = gs.match(A, B)
    assert np.array_equal(out["calls"]["match.best"], best) and np.array_equal(out["calls"]["match.best_d2"], b1.view(np.int32))
    return out


def test_poisoned_scratch(fresh):
    from owlraytracing_amd import _debug_lib
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    try:
        for byte in BYTES:
            assert _debug_lib.poison(eng, _debug_lib.POISON_ALL, byte, WORKSPACE) >= WORKSPACE
            same(both(eng), fresh["calls"], "after poison 0x%02X" % byte)
    finally:
        eng.close()


def test_between_other_calls_and_after_other_workspaces(fresh):
    from owlraytracing_amd.trueknn import TrueKNN

    Q = fresh["Q"]
    eng = TrueKNN(device=0)
    try:
        same(both(eng), fresh["calls"], "before the build")
        eng.build(fresh["P"])
        same(both(eng), fresh["calls"], "on a fresh tree")
        same(others(eng, Q), fresh["others"], "solve and knn after the two calls")
        same(both(eng), fresh["calls"], "after solve and knn")
        big = np.random.default_rng(4).random((40000, 3), dtype=np.float32)
        assert eng.mean_shift_modes(0.1, seeds=big, max_iterations=2)["info"]["walks"] >= len(big)
        same(both(eng), fresh["calls"], "after a call with a larger workspace")
        eng.knn(Q[:2], k=1)
        same(both(eng), fresh["calls"], "after a call with a small workspace")
        same(others(eng, Q), fresh["others"], "solve and knn at the end")
    finally:
        eng.close()
