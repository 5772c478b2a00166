"""tknnMeanShift and the state that carries from one call to the next (tests/test_engine_state_gpu.py's rule, for the new call): the
call gives the same answer, bit for bit, on a fresh engine, after its scratch was poisoned, after unrelated calls on the same engine
and after a call of its own with a larger workspace; and those calls give what they gave without a mean shift before them."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BYTES = (0x00, 0xFF, 0x5A)
WORKSPACE = 4 << 20  # more than the calls here need: their layouts lie wholly inside the poisoned bytes
KERNELS = ("flat", "gauss")
ARRAYS = ("modes", "counts", "wsum", "shift", "iterations", "status")
FALLBACK = "TKNN_MEANSHIFT_FORCE_FALLBACK"


def case():
    rng = np.random.default_rng(12)
    P = rng.uniform(0, 1, size=(3000, 3)).astype(np.float32)
    S = rng.uniform(0, 1, size=(1300, 3)).astype(np.float32)
    S[5, 0] = np.nan
    S[9] = [4, 4, 4]
    Q = rng.uniform(0, 1, size=(500, 3)).astype(np.float32)
    big = rng.uniform(0, 1, size=(20000, 3)).astype(np.float32)
    return P, S, Q, big


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


def shift(eng, kernel, S, own=False):
    bw = 0.1 if kernel == "flat" else 0.04
    r = eng.mean_shift_modes(bw, seeds=None if own else S, kernel=kernel, max_iterations=7)
    out = {k: r[k].cpu().numpy() for k in ARRAYS}
    for k in ("modes", "wsum", "shift"):
        out[k] = out[k].view(np.int32)
    i = r["info"]
    out["info"] = np.int64([i["iterations"], i["walks"], i["converged"], i["empty"], i["running"], i["invalid"]])
    return out


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
    P, S, Q, big = case()
    out = {}
    for kernel in KERNELS:
        for fallback in (False, True):
            eng = engine(P)
            with forced(fallback):
                out[kernel, fallback] = shift(eng, kernel, S)
            eng.close()
            info = out[kernel, fallback]["info"]
            assert info[0] >= 2 and info[1] < 1300 * info[0] and info[3] == 1 and info[5] == 1, "several passes, a shrinking list, an EMPTY and an INVALID seed"
    eng = engine(P)
    out["own"] = shift(eng, "flat", S, own=True)
    eng.close()
    eng = engine(P)
    out["others"] = others(eng, Q)
    eng.close()
    return out


@pytest.mark.parametrize("fallback", [False, True])
@pytest.mark.parametrize("kernel", KERNELS)
def test_poisoned_scratch(fresh, kernel, fallback):
    from owlraytracing_amd import _debug_lib

    P, S, Q, big = case()
    eng = engine(P)
    try:
        for byte in BYTES:
            assert _debug_lib.poison(eng, _debug_lib.POISON_ALL, byte, WORKSPACE) >= WORKSPACE
            with forced(fallback):
                same(shift(eng, kernel, S), fresh[kernel, fallback], "after poison 0x%02X" % byte)
        assert _debug_lib.poison(eng, _debug_lib.POISON_ALL, 0xA5, WORKSPACE) >= WORKSPACE
        same(shift(eng, "flat", S, own=True), fresh["own"], "the own points after poison")
    finally:
        eng.close()


@pytest.mark.parametrize("kernel", KERNELS)
def test_between_other_calls_and_after_a_larger_workspace(fresh, kernel):
    P, S, Q, big = case()
    eng = engine(P)
    try:
        same(others(eng, Q), fresh["others"], "the other calls on a fresh engine")
        same(shift(eng, kernel, S), fresh[kernel, False], "mean shift after solve, knn and radius_reduce")
        same(others(eng, Q), fresh["others"], "solve, knn and radius_reduce after a mean shift")
        same(shift(eng, kernel, S), fresh[kernel, False], "mean shift again")
        other = KERNELS[1 - KERNELS.index(kernel)]
        same(shift(eng, other, S), fresh[other, False], "the other kernel after this one")
        # a call with fifteen times the seeds lays a larger layout over the workspace; the small one after it answers as before
        large = eng.mean_shift_modes(0.1, seeds=big, max_iterations=3)
        assert large["info"]["walks"] >= len(big)
        same(shift(eng, kernel, S), fresh[kernel, False], "mean shift after a call with a larger workspace")
        same(shift(eng, "flat", S, own=True), fresh["own"], "the own points after external seeds")
        same(others(eng, Q), fresh["others"], "the other calls at the end")
    finally:
        eng.close()
