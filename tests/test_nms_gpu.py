"""TrueKNN.radius_nms (tknnRadiusNms, include/owlknn_nms.h) against tests/nms_spec.py: keep, cover and counts are the sequential
loop's, exactly, through the team walk and through the lane kernel; the rounds never exceed the longest chain of dominators."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import nms_spec as ns  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = sorted(ns.CASES)


@pytest.fixture(scope="module")
def eng():
    from owlraytracing_amd.trueknn import TrueKNN

    e = TrueKNN(device=0)
    yield e
    e.close()


def build(eng, c):
    eng.build(c["P"], ids=c["ids"], batch=c["batch"], num_batches=c["num_batches"])


def run(eng, c, **kw):
    r = eng.radius_nms(c["r"], scores=c["scores"], by_name=c["by_name"], **kw)
    out = {k: v.cpu().numpy() for k, v in r.items() if k != "info"}
    out["info"] = r["info"]
    return out


def same(got, want):
    assert np.array_equal(got["counts"], want["counts"]), "counts differ"
    assert np.array_equal(got["keep"], want["keep"]), "keep differs"
    assert np.array_equal(got["cover"], want["cover"]), "cover differs"


def names_of(c):
    return np.arange(len(c["P"]), dtype=np.int64) if c["ids"] is None else np.asarray(c["ids"], np.int64)


@pytest.mark.parametrize("name", NAMES)
def test_equals_the_sequential_loop(eng, name, monkeypatch):
    c, want, deepest = ns.case(name), ns.want(name), ns.max_depth(name)
    build(eng, c)
    got = run(eng, c)
    same(got, want)
    info = got["info"]
    print(name, "rounds", info["rounds"], "depth", deepest, "kept", info["kept"], "eligible", info["eligible"], "fallback", info["fallback_items"])
    assert got["keep"].dtype == np.bool_ and got["idx"].dtype == np.int64
    assert np.array_equal(got["idx"], names_of(c)[want["keep"]])
    assert info["kept"] == want["counts"].sum() and info["eligible"] == want["eligible"] and info["bad_scores"] == want["bad_scores"]
    assert 1 <= info["rounds"] <= deepest
    assert info["solve_ms"] > 0 and info["point_tests"] >= 0 and info["node_tests"] >= 0
    # a second call gives the same
    again = run(eng, c)
    same(again, got)
    assert np.array_equal(again["idx"], got["idx"])
    # without the cover pass
    bare = run(eng, c, want_cover=False)
    assert "cover" not in bare and np.array_equal(bare["keep"], want["keep"]) and np.array_equal(bare["counts"], want["counts"])
    # every walk on the lane kernel
    monkeypatch.setenv("TKNN_NMS_FORCE_FALLBACK", "1")
    lane = run(eng, c)
    same(lane, want)
    assert lane["info"]["fallback_items"] == want["eligible"] == lane["info"]["eligible"]
    assert 1 <= lane["info"]["rounds"] <= deepest


@pytest.mark.parametrize("name", NAMES)
def test_raw_call_writes_only_its_rows(eng, name):
    import torch

    from owlraytracing_amd import _nms_lib

    c, want = ns.case(name), ns.want(name)
    build(eng, c)
    n, B, guard = len(c["P"]), eng.num_clouds, 512
    dev = eng.device
    keep = torch.full((n + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    cover = torch.full((n + 2 * guard,), -7, dtype=torch.int32, device=dev)
    counts = torch.full((B + 2 * guard,), -7, dtype=torch.int32, device=dev)
    scores = None
    if c["scores"] is not None:
        scores = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device=dev)
        scores[guard:guard + n] = torch.from_numpy(np.ascontiguousarray(c["scores"])).to(dev)
    o = _nms_lib.RadiusNmsOptions()
    o.radius, o.flags = float(c["r"]), _nms_lib.NMS_BY_NAME if c["by_name"] else 0
    o.d_scores = None if scores is None else scores[guard:].data_ptr()
    o.d_keep, o.d_cover, o.d_counts = keep[guard:].data_ptr(), cover[guard:].data_ptr(), counts[guard:].data_ptr()
    info = _nms_lib.RadiusNmsInfo()
    with torch.cuda.device(dev):
        rc = _nms_lib.load().tknnRadiusNms(eng._h, ctypes.byref(o), ctypes.byref(info), eng._stream())
    assert rc == 0, _nms_lib.load().tknnLastError()
    assert np.array_equal(keep[guard:guard + n].cpu().numpy(), want["keep"].astype(np.uint8))
    assert np.array_equal(cover[guard:guard + n].cpu().numpy(), want["cover"])
    assert np.array_equal(counts[guard:guard + B].cpu().numpy(), want["counts"])
    assert (keep[:guard] == 0xA5).all() and (keep[guard + n:] == 0xA5).all(), "d_keep: written outside its n bytes"
    assert (cover[:guard] == -7).all() and (cover[guard + n:] == -7).all(), "d_cover: written outside its n words"
    assert (counts[:guard] == -7).all() and (counts[guard + B:] == -7).all(), "d_counts: written outside its B words"
    assert info.kept == want["counts"].sum() and info.eligible == want["eligible"] and info.bad_scores == want["bad_scores"]


def test_other_clouds_do_not_suppress(eng):
    # every cloud of these cases lies in the same unit cube: a cloud's result is that of the cloud alone
    for name in ("straddle", "clouds"):
        c = ns.case(name)
        build(eng, c)
        got = run(eng, c)
        for b in range(c["num_batches"]):
            rows = np.flatnonzero(c["batch"] == b)
            alone = ns.brute(c["P"][rows], c["r"], ids=rows)
            assert np.array_equal(got["keep"][rows], alone["keep"]) and np.array_equal(got["cover"][rows], alone["cover"])
            assert got["counts"][b] == alone["counts"][0]


def test_knn_and_the_tree_are_left_alone(eng):
    c = ns.case("uniform8000")
    build(eng, c)
    before = eng.knn(k=8)
    tree_before = eng.export_tree_ex()
    same(run(eng, c), ns.want("uniform8000"))
    after = eng.knn(k=8)
    assert np.array_equal(before["idx"].cpu().numpy(), after["idx"].cpu().numpy())
    assert np.array_equal(before["dist"].cpu().numpy().view(np.int32), after["dist"].cpu().numpy().view(np.int32))
    tree_after = eng.export_tree_ex()
    for name, a in tree_before.items():
        assert np.array_equal(np.asarray(a), np.asarray(tree_after[name])), name


def test_front_end_and_one_shot(eng):
    import torch

    import owlraytracing_amd
    from owlraytracing_amd.trueknn import radius_nms as one_shot

    c, want = ns.case("nan"), ns.want("nan")
    build(eng, c)
    method = run(eng, c)
    for call in (one_shot, owlraytracing_amd.radius_nms):
        got = call(c["P"], c["r"], scores=c["scores"], batch=c["batch"])
        same(got, want)
        assert np.array_equal(got["idx"], method["idx"]) and got["info"]["kept"] == method["info"]["kept"]
    # scores as a tensor on the device; scores of the wrong length; scores together with by_name
    got = eng.radius_nms(c["r"], scores=torch.from_numpy(np.ascontiguousarray(c["scores"])).to(eng.device))
    assert np.array_equal(got["keep"].cpu().numpy(), want["keep"])
    with pytest.raises(ValueError):
        eng.radius_nms(c["r"], scores=c["scores"][:-1])
    plain = ns.case("planar")
    got = one_shot(plain["P"], plain["r"])
    same(got, ns.want("planar"))
    # max_rounds below the need: TKNN_E_STATE; at the depth: enough
    from owlraytracing_amd._lib import TknnError

    line = ns.case("line_scored")
    build(eng, line)
    with pytest.raises(TknnError) as err:
        run(eng, line, max_rounds=1)
    assert err.value.code == -3 and "max_rounds" in str(err.value)
    same(run(eng, line, max_rounds=ns.LINE_POINTS), ns.want("line_scored"))
