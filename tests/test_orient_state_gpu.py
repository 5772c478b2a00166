"""tknnOrientNormals and the state that carries from one call to the next (tests/test_engine_state_gpu.py's rule, for the new call):
the call gives the same bits on a fresh engine, after its scratch was poisoned, after unrelated calls on the same engine and after
calls with a larger or smaller workspace; and a solve, a knn and an emst give what they gave without an orientation before them."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import orient_spec as osp  # noqa: E402

pytestmark = pytest.mark.gpu

BYTES = (0x00, 0xFF, 0x5A)
WORKSPACE = 8 << 20  # more than the calls here need: their layouts lie wholly inside the poisoned bytes
NAME = "sphere_noisy"


def engine(P):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(P)
    return eng


def describe(eng, emst=True):
    c, _ = osp.case(NAME)
    r = eng.orient_normals(c["N"], k=c["k"], emst=emst, want=("normals", "flip", "components", "tree"))
    out = {k: r[k].cpu().numpy() for k in ("flip", "components", "u", "v")}
    out["normals"], out["w"] = r["normals"].cpu().numpy().view(np.uint32), r["w"].cpu().numpy().view(np.uint32)
    out["info"] = np.int64([r["info"][k] for k in ("candidates", "tree_edges", "components", "excluded", "flipped", "rounds")])
    return out


def others(eng, Q):
    """An unrelated solve, knn (external and own points) and emst; their outputs as bits."""
    s = eng.solve(5, 0.05)
    k = eng.knn(Q, k=3)
    own = eng.knn(k=4)
    e = eng.emst(want_components=True)
    return {"solve.idx": s["idx"].cpu().numpy(), "solve.dist": s["dist"].cpu().numpy().view(np.int32), "knn.idx": k["idx"].cpu().numpy(),
            "knn.dist": k["dist"].cpu().numpy().view(np.int32), "own.idx": own["idx"].cpu().numpy(), "own.dist": own["dist"].cpu().numpy().view(np.int32),
            "emst.u": e["u"].cpu().numpy(), "emst.v": e["v"].cpu().numpy(), "emst.w": e["w"].cpu().numpy().view(np.int32), "emst.components": e["components"].cpu().numpy()}


def same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert np.array_equal(a[name], b[name]), "%s: %s differs" % (what, name)


@pytest.fixture(scope="module")
def fresh():
    c, want = osp.case(NAME)
    Q = np.random.default_rng(3).random((300, 3), dtype=np.float32)
    out = {}
    for emst in (True, False):
        eng = engine(c["P"])
        out[emst] = describe(eng, emst)
        eng.close()
    assert np.array_equal(out[True]["normals"], want["normals"].view(np.uint32)) and np.array_equal(out[True]["u"], want["u"])
    eng = engine(c["P"])
    out["others"] = others(eng, Q)
    eng.close()
    out["Q"] = Q
    return out


@pytest.mark.parametrize("emst", [True, False])
def test_poisoned_scratch(fresh, emst):
    from owlraytracing_amd import _debug_lib

    eng = engine(osp.case(NAME)[0]["P"])
    try:
        for byte in BYTES:
            assert _debug_lib.poison(eng, _debug_lib.POISON_ALL, byte, WORKSPACE) >= WORKSPACE
            same(describe(eng, emst), fresh[emst], "after poison 0x%02X" % byte)
    finally:
        eng.close()


def test_between_other_calls_and_after_other_workspaces(fresh):
    c, _ = osp.case(NAME)
    Q = fresh["Q"]
    eng = engine(c["P"])
    try:
        same(others(eng, Q), fresh["others"], "the other calls on a fresh engine")
        same(describe(eng), fresh[True], "orient_normals after solve, knn and emst")
        same(others(eng, Q), fresh["others"], "solve, knn and emst after an orient_normals")
        same(describe(eng, False), fresh[False], "orient_normals without the EMST's records, on a used engine")
        same(describe(eng), fresh[True], "orient_normals again")
        # a call with many times the queries lays a larger layout over the workspace, a tiny one a smaller; the call answers as before
        big = np.random.default_rng(4).random((40000, 3), dtype=np.float32)
        assert eng.knn(big, k=16)["info"]["total"] > 0
        same(describe(eng), fresh[True], "orient_normals after a call with a larger workspace")
        eng.knn(Q[:2], k=1)
        same(describe(eng), fresh[True], "orient_normals after a call with a small workspace")
        same(others(eng, Q), fresh["others"], "the other calls at the end")
    finally:
        eng.close()
