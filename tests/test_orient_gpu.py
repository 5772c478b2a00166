"""tknnOrientNormals (include/owlknn_orient.h) against its numpy spec (tests/orient_spec.py), bit for bit: normals, flips, components,
the forest's records and their tails, the info counts; in place equals out of place; two runs agree; the result does not depend on the
input's signs; the wrapper under the guard of tests/guarded_outputs.py; the one-shot helper."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import emst_spec as em  # noqa: E402
import orient_spec as osp  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 512  # entries behind every output that the call must leave alone
INF_BITS = 0x7F800000


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def engine(c):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(c["P"], ids=c["ids"])
    return eng


def raw(eng, c, normals=None, in_place=False, **kw):
    """The call through its C ABI, every output given and followed by PAD entries of -7: (rc, {name: numpy}, info)."""
    import torch

    from owlraytracing_amd import _orient_lib

    dev, n = eng.device, len(c["P"])
    N = torch.from_numpy(np.ascontiguousarray(c["N"] if normals is None else normals, np.float32)).to(dev)
    out = {"normals": torch.full((n * 3 + PAD,), -7.0, dtype=torch.float32, device=dev), "flip": torch.full((n + PAD,), 249, dtype=torch.uint8, device=dev),
           "component": torch.full((n + PAD,), -7, dtype=torch.int32, device=dev), "u": torch.full((n - 1 + PAD,), -7, dtype=torch.int32, device=dev),
           "v": torch.full((n - 1 + PAD,), -7, dtype=torch.int32, device=dev), "w": torch.full((n - 1 + PAD,), -7.0, dtype=torch.float32, device=dev)}
    if in_place:
        out["normals"][:n * 3] = N.reshape(-1)
    o = _orient_lib.OrientOptions()
    o.d_normals = out["normals"].data_ptr() if in_place else N.data_ptr()
    o.k, o.flags = c["k"], 0 if c["emst"] else _orient_lib.ORIENT_NO_EMST
    for axis in range(3):
        o.direction[axis] = c["direction"][axis]
    o.d_out_normals, o.d_flip, o.d_component = out["normals"].data_ptr(), out["flip"].data_ptr(), out["component"].data_ptr()
    o.d_u, o.d_v, o.d_w = out["u"].data_ptr(), out["v"].data_ptr(), out["w"].data_ptr()
    for name, value in kw.items():
        setattr(o, name, value)
    info = _orient_lib.OrientInfo()
    rc = _orient_lib.load().tknnOrientNormals(eng._h, ctypes.byref(o), ctypes.byref(info), None)
    torch.cuda.synchronize()
    return rc, {name: t.cpu().numpy() for name, t in out.items()}, info


def check(c, got, info, want):
    n, edges = len(c["P"]), want["tree_edges"]
    assert (info.candidates, info.tree_edges, info.components, info.excluded, info.flipped) == (
        want["candidates"], edges, want["components"], want["excluded"], want["flipped"])
    assert 0 <= info.rounds <= em.round_bound(n)
    assert np.array_equal(got["flip"][:n], want["flip"]), "flips"
    assert np.array_equal(bits(got["normals"][:n * 3]).reshape(n, 3), bits(want["normals"])), "normals, bit for bit"
    assert np.array_equal(got["component"][:n], want["component"]), "components"
    assert np.array_equal(got["u"][:edges], want["u"]) and np.array_equal(got["v"][:edges], want["v"]), "the forest's records"
    assert np.array_equal(bits(got["w"][:edges]), bits(want["w"]))
    assert (got["u"][edges:n - 1] == -1).all() and (got["v"][edges:n - 1] == -1).all() and (bits(got["w"][edges:n - 1]) == INF_BITS).all(), "the tail is filled"
    assert (got["normals"][n * 3:] == -7.0).all() and (got["flip"][n:] == 249).all() and (got["component"][n:] == -7).all()
    assert (got["u"][n - 1:] == -7).all() and (got["v"][n - 1:] == -7).all() and (got["w"][n - 1:] == -7.0).all(), "nothing is written behind an output"


@pytest.mark.parametrize("name", list(osp.CASES))
def test_equals_the_spec_in_place_and_twice(name):
    c, want = osp.case(name)
    eng = engine(c)
    try:
        rc, got, info = raw(eng, c)
        assert rc == 0
        check(c, got, info, want)
        rc, again, info2 = raw(eng, c, in_place=True)  # the second run, and in place
        assert rc == 0
        check(c, again, info2, want)
        for key in got:
            assert np.array_equal(got[key].view(np.uint8), again[key].view(np.uint8)), "%s: two runs, one of them in place, differ" % key
        assert info.rounds == info2.rounds
    finally:
        eng.close()


@pytest.mark.parametrize("name", osp.SIGN_FREE)
def test_the_output_does_not_depend_on_the_input_signs(name):
    c, want = osp.case(name)
    rng = np.random.default_rng(6)
    eng = engine(c)
    try:
        for share in (0.5, 1.0):
            neg = rng.random(len(c["N"])) < share
            N = np.where(neg[:, None], -c["N"], c["N"]).astype(np.float32)
            rc, got, info = raw(eng, c, normals=N)
            assert rc == 0
            n = len(N)
            assert np.array_equal(bits(got["normals"][:n * 3]).reshape(n, 3), bits(want["normals"])), "w uses |c| and negation is exact"
            assert np.array_equal(got["flip"][:n].astype(bool), want["flip"].astype(bool) ^ neg)
            assert np.array_equal(got["u"][:info.tree_edges], want["u"]) and np.array_equal(got["v"][:info.tree_edges], want["v"])
    finally:
        eng.close()


def test_the_wrapper_under_the_guard():
    """TrueKNN.orient_normals with the engine's torch handle replaced by the guard, as tests/test_output_bounds_gpu.py runs the other
    wrappers: every output is written whole -- the records' tails included -- under three fills, nothing is written around one."""
    import torch

    import guarded_outputs as go
    from owlraytracing_amd.trueknn import TrueKNN

    c, want = osp.case("bad_inputs")
    assert want["tree_edges"] < len(c["P"]) - 1 - 40, "the records have a tail"
    stale, account = None, None
    for byte in (0x00, 0xFF, 0x5A):
        e = TrueKNN(device=0)
        g = go.Guarded(torch, byte)
        try:
            e.build(c["P"])
            e._torch = g  # (from here on: the call's own allocations)
            r = e.orient_normals(c["N"], k=c["k"], want=("normals", "flip", "components", "tree"))
            torch.cuda.synchronize()
            assert g.stray() == [], g.stray()
            assert r["info"]["tree_edges"] == want["tree_edges"] and np.array_equal(bits(r["normals"].cpu().numpy()), bits(want["normals"]))
            assert np.array_equal(r["flip"].cpu().numpy(), want["flip"]) and np.array_equal(r["components"].cpu().numpy(), want["component"])
            assert np.array_equal(r["u"].cpu().numpy(), want["u"]) and np.array_equal(r["v"].cpu().numpy(), want["v"]) and np.array_equal(bits(r["w"].cpu().numpy()), bits(want["w"]))
            mine = g.records
            assert [x.spare for x in mine].count(True) == 1 and all(g.as_filled(x.name).all() for x in mine if x.spare)
            filled = {x.name: g.as_filled(x.name, unit=1 if x.dtype == torch.uint8 else 4).cpu().numpy() for x in mine if not x.spare}
            records = [(x.name, x.shape, str(x.dtype)) for x in mine]
        finally:
            e.close()
        assert account is None or account == records
        account = records
        stale = filled if stale is None else {name: stale[name] & filled[name] for name in stale}
    assert len(stale) == 6 and [name for name, left in stale.items() if left.any()] == [], "an output holds a word that no fill changed: never written"


def test_the_wrapper_and_the_one_shot_helper():
    import torch

    import owlraytracing_amd
    from owlraytracing_amd.trueknn import TrueKNN

    c, want = osp.case("tiny17_kbig")
    got = owlraytracing_amd.orient_normals(c["P"], c["N"], k=c["k"], want=("normals", "flip", "components", "tree"))
    assert np.array_equal(bits(got["normals"]), bits(want["normals"])) and np.array_equal(got["flip"], want["flip"])
    assert np.array_equal(got["components"], want["component"]) and np.array_equal(got["u"], want["u"]) and np.array_equal(got["v"], want["v"])
    assert got["info"]["tree_edges"] == want["tree_edges"] and "build_info" in got
    c, want = osp.case("two_spheres_no_emst")
    eng = TrueKNN(device=0)
    try:
        eng.build(c["P"])
        r = eng.orient_normals(c["N"], k=c["k"], emst=False)  # the defaults: normals and flips
        assert sorted(r) == ["flip", "info", "normals"] and r["info"]["components"] == 2
        assert np.array_equal(bits(r["normals"].cpu().numpy()), bits(want["normals"])) and np.array_equal(bits(want["normals"]), bits(c["outward"]))
        N = torch.from_numpy(np.array(c["N"])).to(eng.device)
        r = eng.orient_normals(N, k=c["k"], emst=False, in_place=True, want="normals")
        assert r["normals"] is N and np.array_equal(bits(N.cpu().numpy()), bits(want["normals"]))
        r = eng.orient_normals(c["N"], k=c["k"], want="flip", direction=(0, 0, -1))  # one component, rooted at the lowest point
        assert r["info"]["components"] == 1 and sorted(r) == ["flip", "info"]
        for bad in (dict(want=("normals", "colours")), dict(want=("tree",)), dict(want="flip", in_place=True), dict(direction=(0, 1))):
            with pytest.raises(ValueError):
                eng.orient_normals(N, k=4, **bad)
        for bad in (c["N"][:-1], N.double(), np.zeros((len(c["N"]), 2), np.float32)):
            with pytest.raises(ValueError):
                eng.orient_normals(bad, k=4, in_place=not isinstance(bad, np.ndarray))
    finally:
        eng.close()
