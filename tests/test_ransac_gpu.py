"""TrueKNN.ransac (tknnRansac, include/owlknn_global.h) against its numpy definition (tests/global_spec.py): every trial's status,
every scored trial's inlier count inside [certain, certain + uncertain] of the spec, the best trial, its transform inside the
derived bound, the mask, the stopping rule over one and two batches, the refit, the edges of the input, two runs bit for bit -- and
the pipeline global_registration on two views of one surface."""
import numpy as np
import pytest

import global_spec as gs
import icp_spec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from owlraytracing_amd.trueknn import TrueKNN

    e = TrueKNN(device=0)  # no tree: the call needs none
    yield e
    e.close()


def run(eng, sc, **kw):
    kw.setdefault("seed", gs.TRIAL_SEED)
    r = eng.ransac(sc["S"], sc["P"], sc["pairs"], gs.MAX_DIST, **kw)
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


def plain(r):
    """What two runs must agree on, as comparable values: everything but the times."""
    out = {}
    for k, v in r.items():
        if k.endswith("_ms"):
            continue
        out[k] = v.tobytes() if isinstance(v, np.ndarray) else v
    return out


@pytest.mark.parametrize("n", [3, 4])
def test_every_trial_against_the_spec(eng, n):
    sc, tr = gs.scene_trials(n)
    c = len(sc["pairs"])
    r = run(eng, sc, ransac_n=n, confidence=1.0, max_trials=gs.TRIALS, refit_rounds=0, want_trials=True, want_mask=True)
    status, inl = r["trial_status"], r["trial_inliers"]
    assert r["trials_run"] == gs.TRIALS and r["batches"] == 1
    # the statuses: exactly the spec's, but for the trials the spec leaves open
    held = ~tr["excluded"]
    assert np.array_equal(status[held], tr["status"][held])
    assert ((status >= 0) & (status <= 4)).all()
    assert [r["status_counts"][name] for name in gs.STATUS] == np.bincount(status, minlength=5).tolist()
    # scored: exactly the OK trials, each count between the spec's certain and certain + uncertain
    assert np.array_equal(inl >= 0, status == gs.OK)
    both = (status == gs.OK) & (tr["status"] == gs.OK)
    assert both.sum() >= 5
    assert (inl[both] >= tr["certain"][both]).all() and (inl[both] <= tr["certain"][both] + tr["uncertain"][both]).all()
    assert (inl[status == gs.OK] >= n).all(), "a sample is among its own inliers"
    # the best: most inliers, then the smaller trial
    best = int(np.argmax(inl))
    assert r["best_trial"] == best and r["inliers"] == inl[best] and r["refits_kept"] == 0
    assert both[best]
    T = r["transform"]
    assert np.abs(T[:3, :3] - tr["T"][best][:3, :3]).max() <= tr["bR"][best] and np.abs(T[:3, 3] - tr["T"][best][:3, 3]).max() <= tr["bt"][best]
    assert np.array_equal(T[3], [0, 0, 0, 1])
    # the mask, and what follows from it
    mask = r["mask"].astype(bool)
    assert (mask | ~tr["certain_mask"][best]).all() and (~mask | tr["certain_mask"][best] | tr["uncertain_mask"][best]).all()
    assert mask.sum() == r["inliers"] and r["fitness"] == r["inliers"] / c
    s, p = sc["S"][sc["pairs"][:, 0]], sc["P"][sc["pairs"][:, 1]]
    d2 = ((icp_spec.apply(T, s).astype(np.float64) - p.astype(np.float64)) ** 2).sum(axis=1)
    assert abs(r["inlier_rmse"] - np.sqrt(d2[mask].mean())) <= 1e-12 * r["inlier_rmse"]
    assert r["inliers"] >= 0.5 * c, "the planted motion is found"


def test_degenerate_samples(eng):
    sc = gs.collinear_scene()
    tr = gs.run_trials(sc["S"], sc["P"], sc["pairs"], 3, gs.MAX_DIST, 0.9, gs.TRIAL_SEED, np.arange(256))
    r = run(eng, sc, ransac_n=3, confidence=1.0, max_trials=256, want_trials=True, want_mask=True)
    assert np.array_equal(r["trial_status"], tr["status"]) and (r["trial_status"] == gs.DEGENERATE).sum() > 100
    assert (r["trial_inliers"] == -1).all() and r["best_trial"] == -1 and r["inliers"] == 0 and r["fitness"] == 0 and r["inlier_rmse"] == 0
    assert np.array_equal(r["transform"], np.eye(4)) and not r["mask"].any()
    assert r["status_counts"]["degenerate"] + r["status_counts"]["duplicate"] == 256 == r["trials_run"]


def test_refit(eng):
    sc, _ = gs.scene_trials(3)
    kw = dict(ransac_n=3, confidence=1.0, max_trials=gs.TRIALS, want_mask=True)
    raw, fit = run(eng, sc, refit_rounds=0, **kw), run(eng, sc, refit_rounds=2, **kw)
    assert fit["best_trial"] == raw["best_trial"] and fit["inliers"] >= raw["inliers"] and 0 <= fit["refits_kept"] <= 2
    assert fit["mask"].sum() == fit["inliers"]
    # within the noise of the planted motion: three times its scale on every entry
    assert np.abs(fit["transform"] - sc["T0"]).max() < 3 * sc["noise"]
    assert fit["inlier_rmse"] < 3 * sc["noise"]


def test_stopping_rule_and_batches(eng):
    sc = gs.scene(21, true_share=0.8)
    early = run(eng, sc, confidence=0.999, max_trials=100000, want_trials=True)
    assert early["trials_run"] == gs.BATCH and early["batches"] == 1
    assert (early["trial_status"][gs.BATCH:] == -1).all() and (early["trial_inliers"][gs.BATCH:] == -1).all() and (early["trial_status"][:gs.BATCH] >= 0).all()
    full = run(eng, sc, confidence=1.0, max_trials=5000, want_trials=True)
    assert full["trials_run"] == 5000 and full["batches"] == 2 and (full["trial_status"] >= 0).all()
    assert sum(full["status_counts"].values()) == 5000
    assert np.array_equal(full["trial_status"][:gs.BATCH], early["trial_status"][:gs.BATCH])
    assert np.array_equal(full["trial_inliers"][:gs.BATCH], early["trial_inliers"][:gs.BATCH])
    best = int(np.argmax(full["trial_inliers"]))
    assert full["best_trial"] == best
    assert early["best_trial"] == int(np.argmax(early["trial_inliers"]))
    # a trial's result does not depend on its batch: the partial batch's trials against the spec
    tail = np.arange(gs.BATCH, gs.BATCH + 64)
    tr = gs.run_trials(sc["S"], sc["P"], sc["pairs"], 3, gs.MAX_DIST, 0.9, gs.TRIAL_SEED, tail)
    held = ~tr["excluded"]
    assert np.array_equal(full["trial_status"][tail][held], tr["status"][held])


def test_edges_of_the_input(eng):
    from owlraytracing_amd._lib import TknnError

    sc, _ = gs.scene_trials(3)
    few = dict(sc, pairs=sc["pairs"][:2])
    r = run(eng, few, want_mask=True, want_trials=True, max_trials=100)
    assert r["best_trial"] == -1 and r["trials_run"] == 0 and r["batches"] == 0 and r["inliers"] == 0 and np.array_equal(r["transform"], np.eye(4))
    assert (r["trial_status"] == -1).all() and not r["mask"].any()
    none = dict(sc, pairs=np.zeros((0, 2), np.int32))
    assert run(eng, none)["best_trial"] == -1
    rng = np.random.default_rng(8)
    rand = dict(sc, pairs=np.stack([rng.integers(0, len(sc["S"]), 200), rng.integers(0, len(sc["P"]), 200)], axis=1).astype(np.int32))
    r = run(eng, rand, confidence=1.0, max_trials=2048)
    assert r["best_trial"] == -1 or r["fitness"] < 0.1
    r = run(eng, sc, edge_similarity=0.0, confidence=1.0, max_trials=gs.TRIALS)
    assert r["status_counts"]["edge"] == 0 and r["status_counts"]["far"] > 0
    for bad in ([0, len(sc["P"])], [len(sc["S"]), 0], [-1, 0], [0, -1]):
        pairs = sc["pairs"].copy()
        pairs[137] = bad
        with pytest.raises(TknnError) as err:
            run(eng, dict(sc, pairs=pairs))
        assert err.value.code == -1 and "d_pairs" in str(err.value)


def test_two_runs_agree_bit_for_bit(eng):
    sc, _ = gs.scene_trials(4)
    kw = dict(ransac_n=4, confidence=0.999, max_trials=6000, want_trials=True, want_mask=True)
    a, b = run(eng, sc, **kw), run(eng, sc, **kw)
    assert plain(a) == plain(b)
    assert a["solve_ms"] > 0 and a["sample_ms"] > 0 and a["score_ms"] > 0 and a["refit_ms"] > 0
    from owlraytracing_amd.trueknn import ransac

    one = ransac(sc["S"], sc["P"], sc["pairs"], gs.MAX_DIST, seed=gs.TRIAL_SEED, **kw)
    assert plain(one) == plain(a)


def test_the_tile_mapping_scores_the_same(eng):
    """The scoring kernel that was measured and not adopted (TKNN_RANSAC_SCORE=tile: survivors x record chunks through LDS) gives
    the same bits; 1 500 pairs make it cross a chunk of 1 024 records."""
    import os

    sc = gs.scene(31, c=1500, targets=2000)
    kw = dict(ransac_n=3, confidence=1.0, max_trials=5000, want_trials=True, want_mask=True)
    a = run(eng, sc, **kw)
    before = os.environ.pop("TKNN_RANSAC_SCORE", None)
    os.environ["TKNN_RANSAC_SCORE"] = "tile"
    try:
        b = run(eng, sc, **kw)
    finally:
        os.environ.pop("TKNN_RANSAC_SCORE", None)
        if before is not None:
            os.environ["TKNN_RANSAC_SCORE"] = before
    assert plain(a) == plain(b) and a["inliers"] >= 0.5 * 1500 and a["status_counts"]["ok"] > 64


def test_global_registration_of_two_views():
    """Two views of one sampled surface that share 70 % of their extent (global_spec.two_views: max_dist ten times the sensor noise,
    the source's own part a gap away, so that the shared points are the most inliers a motion near the planted one can have)."""
    from owlraytracing_amd.trueknn import global_registration

    v = gs.two_views()
    max_dist = gs.VIEW_MAX_DIST
    kw = dict(feature_radius=0.15, max_dist=max_dist, seed=3, target_viewpoint=v["view_p"], source_viewpoint=v["view_s"])
    r = global_registration(v["P"], v["S"], **kw)
    assert r["ransac"]["best_trial"] >= 0 and len(r["pairs"]) >= 10
    clean = (v["Q"] - v["T0"][:3, 3]) @ v["T0"][:3, :3]  # the source before its noise
    for T in (r["ransac"]["transform"].numpy(), r["icp"]["transform"].numpy()):
        moved = clean @ T[:3, :3].T + T[:3, 3]
        assert np.linalg.norm(moved - v["Q"], axis=1).max() < max_dist, "the motion is recovered to within max_dist"
    # with icp=True the full-cloud fitness is not below the RANSAC one
    assert r["icp_eval"]["fitness"] >= r["ransac_eval"]["fitness"] > 0.5
    assert r["icp_eval"]["fitness"] == v["shared"] / len(v["S"]), "every shared point, and no other"
    assert r["icp_eval"]["inlier_rmse"] <= r["ransac_eval"]["inlier_rmse"]
    assert np.array_equal(r["transform"].numpy(), r["icp"]["transform"].numpy())
    alone = global_registration(v["P"], v["S"], icp=False, **kw)
    assert "icp" not in alone and np.array_equal(alone["transform"].numpy(), r["ransac"]["transform"].numpy())
