"""TrueKNN.fpfh (tknnFpfh, include/owlknn_fpfh.h) against tests/fpfh_spec.py on every case of the spec: the row lengths against
radius_query, the integer histograms inside the 2 U bound (exact on the plane), SPFH and FPFH inside their derived bounds with the
counts under test fed to the float64 formulas, both forms of the self term, the lane kernel on every row bit for bit in counts, two
calls in a row, and the info."""
import contextlib
import os

import numpy as np
import pytest

import fpfh_spec as fs

pytestmark = pytest.mark.gpu

FALLBACK = "TKNN_FPFH_FORCE_FALLBACK"


@contextlib.contextmanager
def forced(on):
    before = os.environ.pop(FALLBACK, None)
    if on:
        os.environ[FALLBACK] = "1"
    try:
        yield
    finally:
        os.environ.pop(FALLBACK, None)
        if before is not None:
            os.environ[FALLBACK] = before


def engine(c):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(c["P"], ids=c["ids"], batch=c["batch"], num_batches=c["num_batches"])
    return eng


def run(eng, c, **kw):
    r = eng.fpfh(float(c["r"]), normals=c["N"], want_spfh=True, want_counts=True, **kw)
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


@pytest.mark.parametrize("name", fs.CASE_NAMES)
def test_against_the_spec(name):
    import torch

    c = fs.case(name)
    mem, hist, n = c["mem"], c["hist"], len(c["P"])
    eng = engine(c)
    try:
        got = run(eng, c)
        # the rows are radius_query's, less the point itself (a NaN point has no row at all)
        clean = ~np.isnan(c["P"]).any(axis=1)
        rq = eng.radius_query(torch.from_numpy(np.nan_to_num(c["P"], nan=9e9)).to(eng.device), float(c["r"]), sort=False, want_dist=False)
        lens = np.diff(rq["offsets"].cpu().numpy())
        assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"][clean], lens[clean] - 1) and (got["counts"][~clean] == 0).all()
        assert np.array_equal(got["counts"], mem["lengths"])
        # the histograms
        fs.check_counts(got["spfh_counts"], hist)
        print("%s: %d pairs, %d counts off the spec's, U = %d" % (name, hist["pairs"], int(np.abs(got["spfh_counts"] - hist["counts"]).sum()), int(hist["uncertain"].sum())))
        if name.startswith("plane"):
            assert np.array_equal(got["spfh_counts"], hist["counts"]), "the plane's counts are exact"
        assert (got["spfh_counts"][~clean] == 0).all() and (got["spfh"][~clean] == 0).all() and (got["fpfh"][~clean] == 0).all()
        fs.check_floats(got["fpfh"], got["spfh_counts"], mem, True, spfh=got["spfh"])
        i = got["info"]
        assert i["total"] == mem["lengths"].sum() and i["max_row"] == mem["lengths"].max() and i["skipped_pairs"] == hist["skipped"]
        assert i["fallback_items"] in (0, 2 * n), "the walk's rows, or (a tree without a box pyramid) every row of both passes by the lane kernel"
        # PCL's form
        bare = run(eng, c, self_term=False)
        assert np.array_equal(bare["spfh_counts"], got["spfh_counts"]) and np.array_equal(bare["spfh"].view(np.int32), got["spfh"].view(np.int32))
        fs.check_floats(bare["fpfh"], bare["spfh_counts"], mem, False)
        # two calls in a row
        again = run(eng, c)
        assert np.array_equal(again["spfh_counts"], got["spfh_counts"]) and np.array_equal(again["counts"], got["counts"])
        # every row of both passes by the lane kernel: integer sums of one pair function do not depend on the order
        with forced(True):
            lane = run(eng, c)
        assert lane["info"]["fallback_items"] == 2 * n
        assert np.array_equal(lane["spfh_counts"], got["spfh_counts"]) and np.array_equal(lane["counts"], got["counts"])
        assert lane["info"]["total"] == i["total"] and lane["info"]["skipped_pairs"] == i["skipped_pairs"]
        fs.check_floats(lane["fpfh"], lane["spfh_counts"], mem, True, spfh=lane["spfh"], slack=2.0)
    finally:
        eng.close()


def test_inside_boxes_are_streamed():
    """The case `all1100` is there for the range list (test_against_the_spec holds it to the spec like every case, the lane kernel
    included): the first 1024 sorted slots are one box of the pyramid's second level, inside every sphere, so a row notes it, streams
    its slots -- pass 2 with sixteen hits a step -- and tests only the few boxes left, far fewer than the set's 69 leaf blocks."""
    c = fs.case("all1100")
    n = len(c["P"])
    blocks = (n + 15) // 16
    assert n > 1024 and (c["mem"]["lengths"] == n - 1).all(), "every row is the whole set"
    eng = engine(c)
    try:
        one = eng.fpfh(float(c["r"]), normals=c["N"], want_spfh=True)["info"]
        # a walk that streams nothing tests the root's boxes and every leaf block's box: more than `blocks` per row and pass
        assert one["fallback_items"] == 0 and 0 < one["node_tests"] <= 2 * n * blocks // 4, one
        assert one["point_tests"] >= 2 * one["total"] == 2 * n * (n - 1)
    finally:
        eng.close()


def test_normals_from_the_engine_and_the_one_shot():
    from owlraytracing_amd import fpfh
    from owlraytracing_amd.trueknn import TrueKNN

    c = fs.case("sphere1025")
    eng = TrueKNN(device=0)
    eng.build(c["P"])
    try:
        normals = eng.normals(k=16)["normals"]
        a = eng.fpfh(float(c["r"]), normal_k=16)
        b = eng.fpfh(float(c["r"]), normals=normals)
        assert set(a) == {"fpfh", "info"} and np.array_equal(a["fpfh"].cpu().numpy().view(np.int32), b["fpfh"].cpu().numpy().view(np.int32))
        sums = a["fpfh"].cpu().numpy().reshape(-1, 3, 11).sum(axis=2)
        assert np.allclose(sums, 200.0, rtol=1e-4)
        for bad in (dict(), dict(normal_k=16, normal_radius=0.2), dict(normals=normals, normal_k=16)):
            with pytest.raises(ValueError):
                eng.fpfh(float(c["r"]), **bad)
        with pytest.raises(ValueError):
            eng.fpfh(float(c["r"]), normals=normals[:-1])
    finally:
        eng.close()
    one = fpfh(c["P"], float(c["r"]), normals=c["N"], want_counts=True)
    assert isinstance(one["fpfh"], np.ndarray) and one["fpfh"].shape == (1025, 33) and np.array_equal(one["counts"], c["mem"]["lengths"])
