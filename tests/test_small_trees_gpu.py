"""The one-query-per-lane rope walk (csrc/lane_walk.h) on trees where its end conditions can go wrong: n = 1 (the root
is a leaf: the walk starts at a leaf reference), 2 (one node), 3, 17 and 65 points (a last block of one point) -- uniform
points, n copies of one point, and (from three points on) a set with one NaN point.  Every caller of the walk:

| walk                                        | through                                         | against                          |
|---------------------------------------------|-------------------------------------------------|----------------------------------|
| lane_round_kernel, repair_kernel            | solve(kernel=lane), repair_exact                | the C oracle, brute force        |
| query_lane_kernel                           | query under TKNN_QUERY_FORCE_FALLBACK (a child) | tests/query_spec.py              |
| db_core_body, for_each_core_group, db_has_core_neighbour | dbscan (with and without counts), dbscan_noise, dbscan_auto; minPts 1 .. n + 1 | oracle/dbscan_oracle.c |

tknnSolve needs k < n, so a tree of one point is refused with TKNN_E_ARG (test_argument_errors_are_reported_not_hidden);
RT-DBSCAN and tknnQuery take it (test_hip_dbscan_degenerate_sets, the `tiny` set of tests/query_spec.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import ROOT
from owlraytracing_amd import _lib, datasets

sys.path.insert(0, os.path.join(ROOT, "tests"))
import query_spec as qs  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 17, 65]
R0 = 0.05  # a few doublings reach across the unit cube


def _sets(n):
    """(name, xyz): uniform, all coincident, and one NaN point among the uniform ones (the others must be able to have a neighbour)."""
    uniform = datasets.uniform3d(n, seed=100 + n)
    yield "uniform", uniform
    yield "same", np.tile(np.float32([[0.3, 0.4, 0.5]]), (n, 1))
    if n >= 3:
        with_nan = uniform.copy()
        with_nan[n // 2, 1] = np.nan
        yield "one_nan", with_nan


def _ks(limit):
    return sorted({1, (limit + 1) // 2, limit})


def _engine():
    from owlraytracing_amd.trueknn import TrueKNN
    return TrueKNN()


@pytest.mark.parametrize("n", SIZES)
def test_lane_solve_and_repair(n):
    eng = _engine()
    for name, xyz in _sets(n):
        eng.build(xyz)
        good = np.flatnonzero(~np.isnan(xyz).any(axis=1))
        if n == 1:
            with pytest.raises(_lib.TknnError) as e:
                eng.solve(1, R0, kernel=_lib.KERNEL_LANE)
            assert e.value.code == -1  # TKNN_E_ARG: k < n
            continue
        for k in _ks(min(len(good) - 1, 64)):
            what = "n=%d %s k=%d" % (n, name, k)
            ref = oracle.trueknn(xyz[good], k, R0)
            r = eng.solve(k, R0, kernel=_lib.KERNEL_LANE, want_levels=True, max_rounds=ref["rounds"] + 2, allow_unfinished=True)
            assert r["info"]["kernel_used"] == _lib.KERNEL_LANE, what
            assert r["info"]["unfinished"] == n - len(good), what
            lv = r["levels"].cpu().numpy()
            assert (lv[good] >= 0).all() and (np.delete(lv, good) < 0).all(), what
            if len(good) == n:
                assert r["info"]["rounds"] == ref["rounds"], what
            assert np.array_equal(r["idx"].cpu().numpy()[good], good[ref["idx"]]), what
            assert np.array_equal(r["dist"].cpu().numpy()[good].view(np.int32), ref["dist"].view(np.int32)), what
            assert np.array_equal(r["intersections"].cpu().numpy()[good], ref["intersections"]), what
            before = r["idx"].clone(), r["dist"].clone()
            fixed = eng.repair_exact(r, k, R0)
            bi, bd = oracle.bruteforce_knn(xyz[good], k)
            assert np.array_equal(r["idx"].cpu().numpy()[good], good[bi]), what
            assert np.array_equal(r["dist"].cpu().numpy()[good].view(np.int32), bd.view(np.int32)), what
            changed = (before[0] != r["idx"]).any(dim=1) | (before[1].view(dtype=before[0].dtype) != r["dist"].view(dtype=before[0].dtype)).any(dim=1)
            assert fixed == int(changed.sum()), what
    eng.close()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
from owlraytracing_amd.trueknn import TrueKNN
cases = np.load(sys.argv[1])
out = {}
eng = TrueKNN(device=0)
for name in sorted(set(key.split("/")[0] for key in cases.files)):
    eng.build(cases[name + "/P"])
    for k in cases[name + "/ks"]:
        r = eng.query(cases[name + "/Q"], int(k), %r, want_levels=True)
        for field in ("idx", "dist", "intersections", "levels"):
            out["%%s/%%d/%%s" %% (name, k, field)] = r[field].cpu().numpy()
        r = eng.query(cases[name + "/Q"], int(k), %r, exact=True)
        out["%%s/%%d/exact_idx" %% (name, k)] = r["idx"].cpu().numpy()
        out["%%s/%%d/exact_dist" %% (name, k)] = r["dist"].cpu().numpy()
eng.close()
np.savez(sys.argv[2], **out)
print("queries done")
"""


def test_query_lane_kernel_in_a_child_process(tmp_path):
    """TKNN_QUERY_FORCE_FALLBACK=1 sends every query through query_lane_kernel; one child serves all the sets."""
    rng = np.random.default_rng(7)
    cases, arrays = {}, {}
    for n in SIZES:
        for name, P in _sets(n):
            # a point of the set itself, points in and around the cube, one far away
            Q = np.concatenate([P[:1], rng.uniform(-0.2, 1.2, (6, 3)).astype(np.float32), np.float32([[40.0, -3.0, 7.0]])])
            clean = int((~np.isnan(P).any(axis=1)).sum())
            cases["n%02d_%s" % (n, name)] = (P, Q, _ks(min(clean, 64)))
    for key, (P, Q, ks) in cases.items():
        arrays[key + "/P"], arrays[key + "/Q"], arrays[key + "/ks"] = P, Q, np.int32(ks)
    np.savez(tmp_path / "cases.npz", **arrays)
    env = dict(os.environ, TKNN_QUERY_FORCE_FALLBACK="1")
    p = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, R0, R0), str(tmp_path / "cases.npz"), str(tmp_path / "rows.npz")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "queries done" in p.stdout, p.stdout + p.stderr
    got = np.load(tmp_path / "rows.npz")
    for key, (P, Q, ks) in cases.items():
        spec = qs.query_rows(P, Q, ks, R0)
        clean = np.flatnonzero(~np.isnan(P).any(axis=1))
        for k in ks:
            what = "%s k=%d" % (key, k)
            assert (spec[k]["levels"] >= 0).all(), what
            for field in ("idx", "intersections", "levels"):
                assert np.array_equal(got["%s/%d/%s" % (key, k, field)], spec[k][field]), (what, field)
            assert np.array_equal(got["%s/%d/dist" % (key, k)].view(np.int32), spec[k]["dist"].view(np.int32)), what
            want_idx, want_dist = qs.exact_rows(P[clean], Q, k, ids=clean)
            assert np.array_equal(got["%s/%d/exact_idx" % (key, k)], want_idx), what
            assert np.array_equal(got["%s/%d/exact_dist" % (key, k)].view(np.int32), want_dist.view(np.int32)), what


@pytest.mark.parametrize("n", SIZES)
def test_dbscan_counts_noise_and_auto(n):
    eng = _engine()
    for name, xyz in _sets(n):
        eng.build(xyz)
        for eps in (0.05, 0.4, 4.0):  # few neighbours; some; the root is a tight node
            eps = float(np.float32(eps))
            for min_pts in sorted({1, 2, max(n // 2, 1), n, n + 1}):
                what = "n=%d %s eps=%g minPts=%d" % (n, name, eps, min_pts)
                ref = oracle.dbscan(xyz, eps, min_pts)
                got = eng.dbscan(eps, min_pts, want_counts=True)
                assert np.array_equal(got["counts"].cpu().numpy(), ref["counts"]), what
                for r in (got, eng.dbscan(eps, min_pts)):  # (without counts: the count stops at minPts)
                    assert np.array_equal(r["core"].cpu().numpy(), ref["core"]), what
                    assert np.array_equal(r["labels"].cpu().numpy(), ref["labels"]), what
                    assert r["info"]["clusters"] == ref["clusters"], what
                if min_pts > n:
                    assert not ref["core"].any(), what
                noise = eng.dbscan_noise(eps, min_pts)
                assert np.array_equal(noise["noise"].cpu().numpy(), ref["labels"] < 0), what
                assert noise["count"] == int((ref["labels"] < 0).sum()), what
                try:
                    want = oracle.dbscan_auto(xyz, eps, min_pts, 0.5, max_rounds=8)
                except oracle.OracleError:  # minPts above what any eps gives: the rounds run out
                    with pytest.raises(_lib.TknnError):
                        eng.dbscan_auto(eps, min_pts, 0.5, max_rounds=8)
                    assert min_pts > (~np.isnan(xyz).any(axis=1)).sum(), what
                    continue
                auto = eng.dbscan_auto(eps, min_pts, 0.5, max_rounds=8)
                info = auto["info"]
                assert (info["rounds"], info["eps"], info["noise"], info["clusters"]) == (want["rounds"], want["eps"], want["noise"], want["clusters"]), what
                assert np.array_equal(auto["labels"].cpu().numpy(), want["labels"]), what
                assert np.array_equal(auto["core"].cpu().numpy(), want["core"]), what
    eng.close()
