"""tknnSegmentPlane (include/owlknn_plane.h) against its numpy spec (tests/plane_spec.py): the status and the inlier count of every
trial, the best trial, the counts, the mask, the rows and their -1 tail, the fp32 plane and the output plane bit for bit, with the
walk of the box pyramid and with TKNN_PLANE_FORCE_FALLBACK=1, the two paths and two runs agreeing bit for bit; the refit's plane to
the header's tolerance and everything that follows from the reported fp32 plane exactly; pruning as a condition; segment_planes on
three planes; the wrapper under the guard of tests/guarded_outputs.py; the one-shot helper."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_spec as ps  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 512  # entries behind every output that the call must leave alone
F = np.float32
ENV = "TKNN_PLANE_FORCE_FALLBACK"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def engine(P):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(np.array(P))  # (a copy: the cases' arrays are read-only)
    return eng


def raw(eng, c, fallback=False, **kw):
    """The call through its C ABI, every output given and followed by PAD entries of -7 (249 in the mask): (rc, {name: numpy}, info)."""
    import torch

    from owlraytracing_amd import _plane_lib

    dev, n, trials = eng.device, len(c["P"]), c["trials"]
    out = {"mask": torch.full((n + PAD,), 249, dtype=torch.uint8, device=dev), "rows": torch.full((n + PAD,), -7, dtype=torch.int32, device=dev),
           "status": torch.full((trials + PAD,), -7, dtype=torch.int32, device=dev), "inliers": torch.full((trials + PAD,), -7, dtype=torch.int32, device=dev)}
    active = None if c["active"] is None else torch.from_numpy(np.ascontiguousarray(c["active"], np.uint8)).to(dev)
    o = _plane_lib.PlaneOptions()
    o.d_active = None if active is None else active.data_ptr()
    o.distance_threshold, o.max_trials, o.confidence, o.seed, o.refit_rounds = c["thr"], trials, c["confidence"], c["seed"], c["refit_rounds"]
    if c["axis"] is not None:
        for i in range(3):
            o.axis[i] = c["axis"][i]
        o.min_cos = c["min_cos"]
    o.d_inlier_mask, o.d_inlier_rows, o.d_trial_status, o.d_trial_inliers = (out[k].data_ptr() for k in ("mask", "rows", "status", "inliers"))
    for name, value in kw.items():
        setattr(o, name, value)
    info = _plane_lib.PlaneInfo()
    old = os.environ.pop(ENV, None)
    if fallback:
        os.environ[ENV] = "1"
    try:
        rc = _plane_lib.load().tknnSegmentPlane(eng._h, ctypes.byref(o), ctypes.byref(info), None)
        torch.cuda.synchronize()
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old
    return rc, {name: t.cpu().numpy() for name, t in out.items()}, info


def check_final(c, want, got, info, normal, anchor):
    """Everything that follows from the fp32 plane (normal, anchor), exactly; and nothing behind an output."""
    n, cc = len(c["P"]), want["active"]
    ev = ps.evaluate(c["P"], want["A"], normal, anchor, c["thr"])
    plane, sign = ps.output_plane(normal, anchor, c["axis"])
    assert np.array_equal(bits(list(info.normal)), bits(F(sign) * np.asarray(normal, F))) and np.array_equal(bits(list(info.anchor)), bits(anchor)), "the fp32 plane"
    assert np.array_equal(np.array(list(info.plane)).view(np.uint64), plane.view(np.uint64)), "the output plane, bit for bit"
    assert info.inliers == ev["inliers"] and info.fitness == ev["inliers"] / cc
    assert abs(info.inlier_rmse - ev["rmse"]) <= (ev["inliers"] + 2) * 2.0 ** -53 * ev["rmse"], "the header's bound for another order of the sum"
    assert np.array_equal(got["mask"][:n], ev["mask"]), "the mask"
    assert np.array_equal(got["rows"][:ev["inliers"]], ev["rows"]) and (got["rows"][ev["inliers"]:n] == -1).all(), "the rows ascending, then -1"
    return ev


def check(c, want, got, info, fallback):
    n, cc, trials = len(c["P"]), want["active"], c["trials"]
    assert (info.active, info.trials_run, info.batches, info.best_trial) == (cc, want["trials_run"], want["batches"], want["best_trial"])
    assert list(info.status_counts) == want["status_counts"].tolist()
    assert np.array_equal(got["status"][:trials], want["status"]), "the status of every trial, -1 where not run"
    assert np.array_equal(got["inliers"][:trials], want["inliers"]), "the inlier count of every trial, -1 where not scored"
    assert (got["mask"][n:] == 249).all() and (got["rows"][n:] == -7).all() and (got["status"][trials:] == -7).all() and (got["inliers"][trials:] == -7).all(), \
        "nothing is written behind an output"
    scored = want["scored"]
    if fallback or n <= 64:
        assert (info.point_tests, info.lane_rows, info.node_tests, info.boxes_counted) == (cc * scored, cc * scored, 0, 0)
    else:
        assert info.lane_rows == 0 and info.point_tests + info.boxes_counted <= cc * scored and (info.node_tests > 0) == (scored > 0)
    if want["best_trial"] < 0:
        assert list(info.plane) == [0.0] * 4 and list(info.normal) == [0.0] * 3 and list(info.anchor) == [0.0] * 3
        assert (info.inliers, info.fitness, info.inlier_rmse, info.refits_kept) == (0, 0.0, 0.0, 0)
        assert (got["mask"][:n] == 0).all() and (got["rows"][:n] == -1).all()
        return
    best = check_final(c, want, got, info, want["normal"], want["anchor"]) if c["refit_rounds"] == 0 else None
    if best is not None:
        assert info.refits_kept == 0 and best["inliers"] == want["inliers"][want["best_trial"]], "the evaluation counts what the score counted"


def same(a, b, ia, ib, what):
    for key in a:
        assert np.array_equal(a[key], b[key]), "%s: %s differs" % (what, key)
    for field in ("plane", "normal", "anchor", "status_counts"):
        assert list(getattr(ia, field)) == list(getattr(ib, field)), "%s: info.%s differs" % (what, field)
    for field in ("fitness", "inlier_rmse", "inliers", "active", "best_trial", "trials_run", "batches", "refits_kept"):
        assert getattr(ia, field) == getattr(ib, field), "%s: info.%s differs" % (what, field)


EXACT = [name for name in ps.CASES if not name.endswith("_refit")]


@pytest.mark.parametrize("name", EXACT)
def test_equals_the_spec_on_both_paths_and_twice(name):
    c, want = ps.case(name)
    eng = engine(c["P"])
    try:
        rc, got, info = raw(eng, c)
        assert rc == 0
        check(c, want, got, info, False)
        rc, swept, info_s = raw(eng, c, fallback=True)
        assert rc == 0
        check(c, want, swept, info_s, True)
        same(got, swept, info, info_s, "the walk and the fallback")
        rc, again, info2 = raw(eng, c)
        assert rc == 0
        same(got, again, info, info2, "two runs")
        assert (info.node_tests, info.point_tests, info.boxes_counted) == (info2.node_tests, info2.point_tests, info2.boxes_counted)
        if name == "wide":
            assert info.boxes_counted > 0 and info.inliers == want["active"], "the inside rule ran: whole boxes were counted by arithmetic"
            assert info.boxes_counted == want["active"] * want["scored"] and info.point_tests == 0, "every top-level box lies inside such a slab"
    finally:
        eng.close()


def test_outputs_are_optional_and_the_confidence_stops_early():
    c, want = ps.case("plane_clutter")
    c = dict(c, confidence=0.999, trials=4 * ps.BATCH)
    early = ps.segment(c["P"], c["thr"], c["trials"], c["seed"], c["confidence"])
    assert early["trials_run"] == ps.BATCH
    eng = engine(c["P"])
    try:
        rc, got, info = raw(eng, c)
        assert rc == 0
        check(c, early, got, info, False)
        rc, got, info2 = raw(eng, c, d_inlier_mask=None, d_trial_status=None)
        assert rc == 0 and (got["mask"] == 249).all() and (got["status"] == -7).all() and np.array_equal(got["inliers"][:c["trials"]], early["inliers"])
        assert list(info2.plane) == list(info.plane) and info2.inliers == info.inliers
        rc, got, info3 = raw(eng, c, d_inlier_rows=None, d_trial_inliers=None, d_inlier_mask=None, d_trial_status=None)
        assert rc == 0 and all((got[k] == (249 if k == "mask" else -7)).all() for k in got) and list(info3.plane) == list(info.plane)
    finally:
        eng.close()


@pytest.mark.parametrize("name,rounds", [("plane_clutter_refit", 1), ("plane_tight_refit", 1), ("plane_tight_refit", 3)])
def test_the_refit_to_the_headers_tolerance(name, rounds):
    """The first refit's plane is within the header's bound of the spec's; whatever was kept, the reported fp32 plane gives the counts,
    the mask, the rows and the rmse exactly; a refit is kept iff it does not lose inliers (decided here where the spec's count is
    further from the kept count than the rows within the bound of the threshold).  At thr = 0.01 the spec's refit loses a row and is
    rejected; at thr = 0.003 it gains rows and is kept."""
    c, want = ps.case(name)
    c = dict(c, refit_rounds=rounds)
    eng = engine(c["P"])
    try:
        rc, got, info = raw(eng, c)
        assert rc == 0
        check(c, want, got, info, False)
        rc, swept, info_s = raw(eng, c, fallback=True)
        assert rc == 0
        same(got, swept, info, info_s, "the walk and the fallback")
        start = ps.evaluate(c["P"], want["A"], want["normal"], want["anchor"], c["thr"])
        fit = ps.refit(c["P"], start["rows"], ps.scene_centre(c["P"]))
        assert fit is not None and fit["tol_normal"] < 1e-6
        mine = ps.evaluate(c["P"], want["A"], fit["normal"], fit["anchor"], c["thr"])
        reach = float(np.abs(c["P"][want["A"]]).max()) * 3
        band = 3 * fit["tol_normal"] * reach + 3 * fit["tol_anchor"] + 8 * 2.0 ** -24 * reach
        d = ps.distances(fit["normal"], fit["anchor"], c["P"][want["A"]])[0].astype(np.float64)
        unsure = int((np.abs(d - c["thr"]) <= band).sum())
        print("refit: start %d inliers, spec's refit %d, unsure %d, kept %d, tol_normal %.3g" % (start["inliers"], mine["inliers"], unsure, info.refits_kept, fit["tol_normal"]))
        assert 0 <= info.refits_kept <= rounds
        if mine["inliers"] - unsure >= start["inliers"]:
            assert info.refits_kept >= 1, "a refit that does not lose inliers is kept"
        if mine["inliers"] + unsure < start["inliers"]:
            assert info.refits_kept == 0, "a refit that loses inliers is rejected"
        normal, anchor = np.array(list(info.normal), F), np.array(list(info.anchor), F)
        if info.refits_kept == 0:
            final = check_final(c, want, got, info, want["normal"], want["anchor"])
        else:
            final = check_final(c, want, got, info, normal, anchor)
            assert final["inliers"] >= start["inliers"]
        if name == "plane_tight_refit":
            assert info.refits_kept >= 1 and mine["inliers"] - unsure >= start["inliers"], "the case where a refit is kept"
        if info.refits_kept == 1:
            s = 1.0 if float(normal @ fit["normal"]) > 0 else -1.0
            assert np.abs(s * normal.astype(np.float64) - fit["normal"]).max() <= fit["tol_normal"], "the normal, to the header's bound"
            assert np.abs(anchor.astype(np.float64) - fit["anchor"]).max() <= fit["tol_anchor"], "the anchor, to the header's bound"
    finally:
        eng.close()


def test_the_walk_prunes():
    """Pruning is a condition: on the 65 553-point uniform cube with thr = 0.01 of the edge the walk puts fewer than half of
    c * (scored trials) rows to the distance expression; the forced fallback puts every one.  The share of the tree's 16-point blocks
    whose box meets such a slab, from tests/lbvh_spec.py's rebuild of the sorted order for this seed and these trials' planes, is 0.13
    (0.132 over the first 64 planes; thr was not lowered): below the 0.35 the bound of 0.5 was chosen for."""
    c, want = ps.case("cube65553")
    ok = np.flatnonzero(want["status"] == ps.OK)[:64]
    _, nm, an, _ = ps.trial_planes(c["P"], want["A"], c["seed"], ok)
    share = ps.block_share(c["P"], c["thr"], nm, an)
    print("share of blocks meeting the slab: %.4f" % share)
    assert share < 0.35
    eng = engine(c["P"])
    try:
        rc, got, info = raw(eng, c)
        assert rc == 0
        full = want["active"] * want["scored"]
        print("point_tests %d of %d (%.4f), boxes_counted %d, node_tests %d" % (info.point_tests, full, info.point_tests / full, info.boxes_counted, info.node_tests))
        assert info.point_tests < 0.5 * full and info.lane_rows == 0
        assert info.point_tests >= 0.5 * share * full, "the blocks that meet the slab are tested, active rows and all"
        rc, got, info = raw(eng, c, fallback=True)
        assert rc == 0 and info.point_tests == full == info.lane_rows
    finally:
        eng.close()


def test_segment_planes_finds_three_planes():
    P = ps.three_planes(8209, 11)
    thr, trials, seed = 0.01, ps.TRIALS, 3
    eng = engine(P)
    try:
        planes, labels = eng.segment_planes(thr, max_planes=5, min_inliers=400, num_iterations=trials, confidence=1.0, seed=seed, refit_rounds=0)
        assert len(planes) == 3, "three planes, then clutter below min_inliers"
        labels = labels.cpu().numpy()
        active = np.ones(len(P), np.uint8)
        for i, (plane, rows) in enumerate(planes):
            want = ps.segment(P, thr, trials, seed, 1.0, active)
            ev = ps.evaluate(P, want["A"], want["normal"], want["anchor"], thr)
            rows = rows.cpu().numpy()
            assert np.array_equal(rows, ev["rows"]), "plane %d: the spec's inliers under the same successive mask" % i
            assert np.array_equal(plane.numpy().view(np.uint64), ps.output_plane(want["normal"], want["anchor"])[0].view(np.uint64))
            assert (labels[rows] == i).all() and (labels == i).sum() == len(rows), "labels are consistent with the rows"
            active[rows] = 0
        assert ps.segment(P, thr, trials, seed, 1.0, active)["inliers"].max() < 400 and (labels[active != 0] == -1).all()
        for (plane, _), axis in zip(planes, ((0, 0, 1), (1, 0, 0), (0, 0.5 ** 0.5, 0.5 ** 0.5))):  # 35, 25 and 15 percent of the rows
            assert np.abs(np.abs(plane.numpy()[:3]) - axis).max() < 0.03, (plane, axis)
        mine = np.ones(len(P), bool)
        mine[::3] = False
        kept = mine.copy()
        planes2, labels2 = eng.segment_planes(thr, max_planes=1, min_inliers=1, active=mine, num_iterations=trials, confidence=1.0, seed=seed, refit_rounds=0)
        assert len(planes2) == 1 and np.array_equal(mine, kept) and (labels2.cpu().numpy()[::3] == -1).all(), "the caller's mask stays as it is"
    finally:
        eng.close()


def test_the_wrapper_under_the_guard():
    """TrueKNN.segment_plane with the engine's torch handle replaced by the guard: every output is written whole -- the rows' tail
    included -- under three fills, nothing is written around one, and the results do not depend on the fill."""
    import torch

    import guarded_outputs as go
    from owlraytracing_amd.trueknn import TrueKNN

    c, want = ps.case("nan_inf")
    ev = ps.evaluate(c["P"], want["A"], want["normal"], want["anchor"], c["thr"])
    assert ev["inliers"] < len(c["P"]) - 40, "the rows have a tail"
    stale, account = None, None
    for byte in (0x00, 0xFF, 0x5A):
        e = TrueKNN(device=0)
        g = go.Guarded(torch, byte)
        try:
            e.build(np.array(c["P"]))
            e._torch = g  # (from here on: the call's own allocations)
            r = e.segment_plane(c["thr"], num_iterations=c["trials"], confidence=1.0, seed=c["seed"], refit_rounds=0, want=("plane", "inliers", "mask", "trials"), return_info=True)
            torch.cuda.synchronize()
            assert g.stray() == [], g.stray()
            assert r["info"]["best_trial"] == want["best_trial"] and np.array_equal(r["rows"].cpu().numpy(), ev["rows"]) and np.array_equal(r["mask"].cpu().numpy(), ev["mask"])
            assert np.array_equal(r["trial_status"].cpu().numpy(), want["status"]) and np.array_equal(r["trial_inliers"].cpu().numpy(), want["inliers"])
            assert np.array_equal(r["plane"].numpy().view(np.uint64), ps.output_plane(want["normal"], want["anchor"])[0].view(np.uint64))
            mine = g.records
            assert [x.spare for x in mine].count(True) == 1 and all(g.as_filled(x.name).all() for x in mine if x.spare)
            filled = {x.name: g.as_filled(x.name, unit=1 if x.dtype == torch.uint8 else 4).cpu().numpy() for x in mine if not x.spare}
            records = [(x.name, x.shape, str(x.dtype)) for x in mine]
        finally:
            e.close()
        assert account is None or account == records
        account = records
        stale = filled if stale is None else {name: stale[name] & filled[name] for name in stale}
    assert len(stale) == 4 and [name for name, left in stale.items() if left.any()] == [], "an output holds a word that no fill changed: never written"


def test_the_wrapper_and_the_one_shot_helper():
    import torch

    import owlraytracing_amd
    from owlraytracing_amd.trueknn import TrueKNN

    c, _ = ps.case("axis")
    angle = 0.14  # radians; the wrapper hands the library cos(angle) rounded to fp32: the spec takes the same min_cos
    min_cos = float(F(np.cos(angle)))
    want = ps.segment(c["P"], c["thr"], c["trials"], c["seed"], 1.0, None, c["axis"], min_cos)
    assert 0 < want["status_counts"][ps.ANGLE] < c["trials"] and want["best_trial"] >= 0
    ev = ps.evaluate(c["P"], want["A"], want["normal"], want["anchor"], c["thr"])
    plane, rows = owlraytracing_amd.segment_plane(np.array(c["P"]), c["thr"], num_iterations=c["trials"], confidence=1.0, seed=c["seed"], axis=c["axis"], max_angle=angle, refit_rounds=0)
    assert isinstance(plane, np.ndarray) and plane.shape == (4,) and rows.dtype == np.int32
    assert np.array_equal(rows, ev["rows"]) and np.array_equal(plane.view(np.uint64), ps.output_plane(want["normal"], want["anchor"], c["axis"])[0].view(np.uint64))
    assert plane[2] > 0.99, "turned towards the axis"
    eng = TrueKNN(device=0)
    try:
        eng.build(np.array(c["P"]))
        plane, rows = eng.segment_plane(c["thr"])  # the defaults: Open3D's pair
        assert isinstance(plane, torch.Tensor) and plane.dtype == torch.float64 and rows.dtype == torch.int32 and rows.is_cuda and len(rows) > 1500
        assert abs(float(np.linalg.norm(plane.numpy()[:3])) - 1.0) < 1e-6
        r = eng.segment_plane(c["thr"], want="mask", return_info=True)
        assert sorted(r) == ["info", "mask", "plane"] and int(r["mask"].sum()) == r["info"]["inliers"] and r["info"]["refits_kept"] in (0, 1)
        active = np.zeros(len(c["P"]), np.uint8)
        r = eng.segment_plane(c["thr"], active=active, return_info=True)
        assert r["info"]["active"] == 0 and r["info"]["best_trial"] == -1 and len(r["rows"]) == 0 and r["plane"].tolist() == [0.0] * 4
        for bad in (dict(want="colours"), dict(axis=(0, 0, 1)), dict(max_angle=0.1), dict(axis=(0, 0, 0), max_angle=0.1), dict(active=active[:-1]), dict(active=active.astype(np.float32))):
            with pytest.raises(ValueError):
                eng.segment_plane(c["thr"], **bad)
    finally:
        eng.close()
