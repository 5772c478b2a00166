"""tknnFpfh and the state that carries from one call to the next (tests/test_engine_state_gpu.py's rule, for the new call): the call
gives the same histograms, bit for bit in the counts and inside the bound in the floats, on a fresh engine, after its scratch was
poisoned, after unrelated calls on the same engine and after a call of its own with a larger or smaller workspace; and those calls
give what they gave without an FPFH before them."""
import contextlib
import os

import numpy as np
import pytest

import fpfh_spec as fs

pytestmark = pytest.mark.gpu

BYTES = (0x00, 0xFF, 0x5A)
WORKSPACE = 4 << 20  # more than the calls here need: their layouts lie wholly inside the poisoned bytes
FALLBACK = "TKNN_FPFH_FORCE_FALLBACK"
NAME = "cube1025"


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


def engine(P):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(P)
    return eng


def describe(eng):
    c = fs.case(NAME)
    r = eng.fpfh(float(c["r"]), normals=c["N"], want_spfh=True, want_counts=True)
    out = {k: r[k].cpu().numpy() for k in ("fpfh", "spfh", "spfh_counts", "counts")}
    out["info"] = np.int64([r["info"]["total"], r["info"]["max_row"], r["info"]["skipped_pairs"]])
    return out


def others(eng, Q):
    """An unrelated solve, knn, radius_reduce and mean shift; their outputs as bits."""
    s = eng.solve(5, 0.05)
    k = eng.knn(Q, k=3)
    r = eng.radius_reduce(0.15, queries=Q, weight="epanechnikov")
    m = eng.mean_shift_modes(0.1, seeds=Q, max_iterations=4)
    return {"solve.idx": s["idx"].cpu().numpy(), "solve.dist": s["dist"].cpu().numpy().view(np.int32), "knn.idx": k["idx"].cpu().numpy(),
            "knn.dist": k["dist"].cpu().numpy().view(np.int32), "reduce.wsum": r["wsum"].cpu().numpy().view(np.int32), "reduce.counts": r["counts"].cpu().numpy(),
            "shift.modes": m["modes"].cpu().numpy().view(np.int32), "shift.status": m["status"].cpu().numpy()}


def same(a, b, what):
    """Counts and info bit for bit; the floats inside the bound of the spec, which both sides are held to with the same counts --
    and, the order of a row's additions being the walk's own, in fact equal."""
    assert a.keys() == b.keys()
    for name in a:
        if a[name].dtype == np.float32 and name in ("fpfh", "spfh"):
            continue
        assert np.array_equal(a[name], b[name]), "%s: %s differs" % (what, name)
    if "fpfh" in a:
        c = fs.case(NAME)
        fs.check_floats(a["fpfh"], a["spfh_counts"], c["mem"], True, spfh=a["spfh"])


@pytest.fixture(scope="module")
def fresh():
    c = fs.case(NAME)
    Q = np.random.default_rng(3).random((300, 3), dtype=np.float32)
    out = {}
    for fallback in (False, True):
        eng = engine(c["P"])
        with forced(fallback):
            out[fallback] = describe(eng)
        eng.close()
    assert np.array_equal(out[False]["spfh_counts"], out[True]["spfh_counts"])
    eng = engine(c["P"])
    out["others"] = others(eng, Q)
    eng.close()
    out["Q"] = Q
    return out


@pytest.mark.parametrize("fallback", [False, True])
def test_poisoned_scratch(fresh, fallback):
    from owlraytracing_amd import _debug_lib

    eng = engine(fs.case(NAME)["P"])
    try:
        for byte in BYTES:
            assert _debug_lib.poison(eng, _debug_lib.POISON_ALL, byte, WORKSPACE) >= WORKSPACE
            with forced(fallback):
                same(describe(eng), fresh[fallback], "after poison 0x%02X" % byte)
    finally:
        eng.close()


def test_between_other_calls_and_after_other_workspaces(fresh):
    c = fs.case(NAME)
    Q = fresh["Q"]
    eng = engine(c["P"])
    try:
        same(others(eng, Q), fresh["others"], "the other calls on a fresh engine")
        same(describe(eng), fresh[False], "fpfh after solve, knn, radius_reduce and mean shift")
        same(others(eng, Q), fresh["others"], "solve, knn, radius_reduce and mean shift after an fpfh")
        same(describe(eng), fresh[False], "fpfh again")
        # a call with many times the seeds lays a larger layout over the workspace, a tiny one a smaller; the call answers as before
        big = np.random.default_rng(4).random((40000, 3), dtype=np.float32)
        assert eng.mean_shift_modes(0.1, seeds=big, max_iterations=2)["info"]["walks"] >= len(big)
        same(describe(eng), fresh[False], "fpfh after a call with a larger workspace")
        eng.knn(Q[:2], k=1)
        same(describe(eng), fresh[False], "fpfh after a call with a small workspace")
        same(others(eng, Q), fresh["others"], "the other calls at the end")
    finally:
        eng.close()
