"""tknnSegmentPlane and the state that carries from one call to the next (tests/test_engine_state_gpu.py's rule, for the new call):
the call gives the same bits on a fresh engine, after its scratch was poisoned, and after a solve, a knn, a radius_nms and an icp on
the same engine, with the walk and with the forced fallback; it leaves the tree and the solve state as they were -- a knn before and
after gives the same rows, tknnExportTreeEx the same bytes --; and no write lands outside its outputs (guard bands around each)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_spec as ps  # noqa: E402
from test_plane_gpu import ENV, engine, raw  # noqa: E402

pytestmark = pytest.mark.gpu

BYTES = (0x00, 0xFF, 0x5A)
WORKSPACE = 8 << 20  # more than the calls here need: their layouts lie wholly inside the poisoned bytes
NAME = "active_half"  # a mask, so the prefixes matter; 1025 points: two pyramid levels
WANT = ("plane", "inliers", "mask", "trials")


def describe(eng, fallback=False):
    c, _ = ps.case(NAME)
    old = os.environ.pop(ENV, None)
    if fallback:
        os.environ[ENV] = "1"
    try:
        r = eng.segment_plane(c["thr"], num_iterations=c["trials"], confidence=1.0, seed=c["seed"], active=c["active"], refit_rounds=2, want=WANT, return_info=True)
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old
    out = {k: r[k].cpu().numpy() for k in ("rows", "mask", "trial_status", "trial_inliers")}
    out["plane"] = r["plane"].numpy().view(np.uint64)
    out["fp32"] = np.float32(r["info"]["normal"] + r["info"]["anchor"]).view(np.uint32)
    out["rmse"] = np.float64([r["info"]["inlier_rmse"], r["info"]["fitness"]]).view(np.uint64)
    out["info"] = np.int64([r["info"][k] for k in ("inliers", "active", "best_trial", "trials_run", "batches", "refits_kept")] + list(r["info"]["status_counts"].values()))
    return out


def others(eng, Q):
    """An unrelated solve, knn (external and own points), radius_nms and icp; their outputs as bits."""
    s = eng.solve(5, 0.05)
    k = eng.knn(Q, k=3)
    own = eng.knn(k=4)
    nms = eng.radius_nms(0.05)
    icp = eng.icp(Q, 0.2, max_iterations=3)
    return {"solve.idx": s["idx"].cpu().numpy(), "solve.dist": s["dist"].cpu().numpy().view(np.int32), "knn.idx": k["idx"].cpu().numpy(),
            "knn.dist": k["dist"].cpu().numpy().view(np.int32), "own.idx": own["idx"].cpu().numpy(), "own.dist": own["dist"].cpu().numpy().view(np.int32),
            "nms.keep": nms["keep"].cpu().numpy(), "icp.T": icp["transform"].numpy().view(np.uint64)}


def same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert np.array_equal(a[name], b[name]), "%s: %s differs" % (what, name)


@pytest.fixture(scope="module")
def fresh():
    c, want = ps.case(NAME)
    Q = np.random.default_rng(3).random((300, 3), dtype=np.float32)
    out = {}
    for fallback in (False, True):
        eng = engine(c["P"])
        out[fallback] = describe(eng, fallback)
        eng.close()
    same(out[False], out[True], "the walk and the fallback")
    assert np.array_equal(out[False]["trial_inliers"], want["inliers"]) and out[False]["info"][2] == want["best_trial"]
    eng = engine(c["P"])
    out["others"] = others(eng, Q)
    eng.close()
    out["Q"] = Q
    return out


@pytest.mark.parametrize("fallback", [False, True])
def test_poisoned_scratch(fresh, fallback):
    from owlraytracing_amd import _debug_lib

    eng = engine(ps.case(NAME)[0]["P"])
    try:
        for byte in BYTES:
            assert _debug_lib.poison(eng, _debug_lib.POISON_ALL, byte, WORKSPACE) >= WORKSPACE
            same(describe(eng, fallback), fresh[fallback], "after poison 0x%02X" % byte)
    finally:
        eng.close()


def test_between_other_calls_and_the_tree_stays(fresh):
    c, _ = ps.case(NAME)
    Q = fresh["Q"]
    eng = engine(c["P"])
    try:
        tree = eng.export_tree_ex()
        same(others(eng, Q), fresh["others"], "the other calls on a fresh engine")
        same(describe(eng), fresh[False], "segment_plane after solve, knn, radius_nms and icp")
        same(others(eng, Q), fresh["others"], "solve, knn, radius_nms and icp after a segment_plane")
        same(describe(eng, True), fresh[True], "segment_plane by the fallback, on a used engine")
        same(describe(eng), fresh[False], "segment_plane again")
        # a call with many times the queries lays a larger layout over the workspace, a tiny one a smaller; the call answers as before
        big = np.random.default_rng(4).random((40000, 3), dtype=np.float32)
        assert eng.knn(big, k=16)["info"]["total"] > 0
        same(describe(eng), fresh[False], "segment_plane after a call with a larger workspace")
        eng.knn(Q[:2], k=1)
        same(describe(eng), fresh[False], "segment_plane after a call with a small workspace")
        same(others(eng, Q), fresh["others"], "the other calls at the end")
        after = eng.export_tree_ex()
        assert tree.keys() == after.keys()
        for name in tree:
            assert np.array_equal(np.asarray(tree[name]).view(np.uint8) if isinstance(tree[name], np.ndarray) else tree[name],
                                  np.asarray(after[name]).view(np.uint8) if isinstance(after[name], np.ndarray) else after[name]), "the tree's %s changed" % name
    finally:
        eng.close()


def test_the_solve_state_stays():
    """A knn, a segment_plane, the knn again: the rows it gave before, and the rows an engine gives that never segmented."""
    c, _ = ps.case("plane_clutter")
    rows = {}
    for between in (False, True):
        eng = engine(c["P"])
        try:
            first = eng.knn(k=8)
            if between:
                eng.segment_plane(c["thr"], num_iterations=64, want=WANT, return_info=True)
            second = eng.knn(k=8)
            rows[between] = (first["idx"].cpu().numpy(), second["idx"].cpu().numpy(), second["dist"].cpu().numpy().view(np.int32))
            assert np.array_equal(rows[between][0], rows[between][1]), "a knn before and after gives the same rows"
        finally:
            eng.close()
    for a, b in zip(rows[False], rows[True]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["n17", "nan_inf", "n1025"])
def test_no_write_lands_outside_the_outputs(name):
    """Guard bands around every output, as tests/test_output_bounds_gpu.py has them for the older calls: raw() puts 512 entries behind
    each, here every output also starts 512 entries into its allocation."""
    import ctypes

    import torch

    from owlraytracing_amd import _plane_lib

    c, want = ps.case(name)
    eng = engine(c["P"])
    try:
        n, trials, pad = len(c["P"]), c["trials"], 512
        bufs = {"mask": torch.full((pad + n + pad,), 249, dtype=torch.uint8, device=eng.device), "rows": torch.full((pad + n + pad,), -7, dtype=torch.int32, device=eng.device),
                "status": torch.full((pad + trials + pad,), -7, dtype=torch.int32, device=eng.device), "inliers": torch.full((pad + trials + pad,), -7, dtype=torch.int32, device=eng.device)}
        at = {k: t[pad:].data_ptr() for k, t in bufs.items()}
        rc, got, info = raw(eng, c, d_inlier_mask=at["mask"], d_inlier_rows=at["rows"], d_trial_status=at["status"], d_trial_inliers=at["inliers"])
        assert rc == 0 and all((got[k] == (249 if k == "mask" else -7)).all() for k in got), "raw()'s own outputs were not given: untouched"
        torch.cuda.synchronize()
        for k, t in bufs.items():
            size = n if k in ("mask", "rows") else trials
            fill = 249 if k == "mask" else -7
            assert (t[:pad] == fill).all() and (t[pad + size:] == fill).all(), "%s: a write in front of or behind the output" % k
            assert not (t[pad:pad + size] == fill).any(), "%s: a word of the output was left as it was" % k
        assert np.array_equal(bufs["status"][pad:pad + trials].cpu().numpy(), want["status"]) and np.array_equal(bufs["inliers"][pad:pad + trials].cpu().numpy(), want["inliers"])
        assert ctypes.sizeof(_plane_lib.PlaneInfo) == 184
    finally:
        eng.close()
