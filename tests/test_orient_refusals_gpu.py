"""What tknnOrientNormals (include/owlknn_orient.h) refuses, one fault per row and in the header's order, and that a refused call
writes nothing, info included."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import orient_spec as osp  # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, ROUNDS, UNSUPPORTED = -1, -3, -4, -5


def test_error_codes_in_order():
    import re

    import torch

    from owlraytracing_amd import _orient_lib
    from owlraytracing_amd.trueknn import TrueKNN

    with open(os.path.join(ROOT, "include", "owlknn.h")) as f:
        text = f.read()
    for name, code in (("TKNN_E_ARG", ARG), ("TKNN_E_UNSUPPORTED", UNSUPPORTED), ("TKNN_E_STATE", STATE), ("TKNN_E_ROUNDS", ROUNDS)):
        assert int(re.search(r"%s = (-\d+)" % name, text).group(1)) == code, name
    lib = _orient_lib.load()
    c, want = osp.case("lattice")
    P, n = c["P"], len(c["P"])
    eng = TrueKNN(device=0)
    dev = eng.device
    guard = 1024
    N = torch.from_numpy(np.array(c["N"])).to(dev)
    normals = torch.full((n * 3 + guard,), -7.0, dtype=torch.float32, device=dev)
    flip = torch.full((n + guard,), 249, dtype=torch.uint8, device=dev)
    comp = torch.full((n + guard,), -7, dtype=torch.int32, device=dev)
    u = torch.full((n - 1 + guard,), -7, dtype=torch.int32, device=dev)
    v = torch.full((n - 1 + guard,), -7, dtype=torch.int32, device=dev)
    w = torch.full((n - 1 + guard,), -7.0, dtype=torch.float32, device=dev)
    info = _orient_lib.OrientInfo()

    def call(handle=None, options=True, direction=(0, 0, 1), **kw):
        o = _orient_lib.OrientOptions()
        o.d_normals, o.k = N.data_ptr(), 6
        o.d_out_normals, o.d_flip, o.d_component = normals.data_ptr(), flip.data_ptr(), comp.data_ptr()
        o.d_u, o.d_v, o.d_w = u.data_ptr(), v.data_ptr(), w.data_ptr()
        for axis in range(3):
            o.direction[axis] = direction[axis]
        for name, value in kw.items():
            setattr(o, name, value)
        return lib.tknnOrientNormals(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)

    def untouched():
        torch.cuda.synchronize()
        return (bool((normals == -7.0).all()) and bool((flip == 249).all()) and bool((comp == -7).all()) and bool((u == -7).all()) and bool((v == -7).all())
                and bool((w == -7.0).all()) and np.array_equal(N.cpu().numpy().view(np.uint32), c["N"].view(np.uint32)))

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnOrientNormals: "), t
        return t

    info.tree_edges, info.rounds = 99, 98
    # 1. engine and options, no output, d_normals: before the state
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(d_out_normals=None, d_flip=None) == ARG and "no output" in text()
    assert call(d_normals=None) == ARG and "d_normals" in text()
    assert call(d_out_normals=None, d_flip=None, d_normals=None) == ARG and "no output" in text(), "the outputs are asked for first"
    # 2. not built, before the values
    assert call() == STATE and "tknnBuild" in text()
    assert call(k=0) == STATE and call(flags=2) == STATE and call(direction=(0, float("nan"), 0)) == STATE
    eng.build(P)
    assert call(d_normals=None, k=0) == ARG and "d_normals" in text(), "pointers before values"
    # 3. k, flags, direction
    assert call(k=0) == ARG and "k" in text()
    assert call(k=-3) == ARG and call(k=65) == ARG and "k out of range" in text()
    assert call(flags=2) == ARG and "flags" in text()
    assert call(flags=0x80000001) == ARG
    for bad in ((float("nan"), 0, 1), (0, float("inf"), 1), (0, 0, -float("inf"))):
        assert call(direction=bad) == ARG and "direction" in text()
    assert call(k=0, flags=2) == ARG and "k" in text(), "k before the flags"
    # 5. the round guard
    assert call(max_rounds=1) == ROUNDS and "max_rounds" in text()
    assert (info.tree_edges, info.rounds) == (99, 98), "a refused call leaves info alone"
    assert untouched(), "a refused call writes nothing"
    # the call itself, with its options at their edges: k = 64, one output, a cap above the bound
    assert call(max_rounds=1000) == 0 and info.tree_edges == want["tree_edges"] and info.components == 1 and 2 <= info.rounds
    torch.cuda.synchronize()
    assert np.array_equal(flip[:n].cpu().numpy(), want["flip"]) and np.array_equal(normals[:n * 3].cpu().numpy().view(np.uint32).reshape(n, 3), want["normals"].view(np.uint32))
    for t in (normals, flip, comp, u, v, w):
        t.fill_(249 if t is flip else -7)
    assert call(d_out_normals=None, d_component=None, d_u=None, d_v=None, d_w=None, k=64) == 0 and info.candidates == n * 64 + n - 1
    torch.cuda.synchronize()
    assert (normals == -7.0).all() and (comp == -7).all() and (u == -7).all() and (w == -7.0).all() and (flip[n:] == 249).all() and (flip[:n] <= 1).all()
    flip.fill_(249)
    assert call(d_flip=None, d_u=None) == 0
    torch.cuda.synchronize()
    assert (flip == 249).all() and (u == -7).all() and np.array_equal(v[:n - 1].cpu().numpy(), want["v"])
    # n = 1: no edges, one component, the point its own root
    eng.build(P[:1])
    for t in (normals, flip, comp, u, v, w):
        t.fill_(249 if t is flip else -7)
    assert call(direction=(0, 0, -1)) == 0 and (info.tree_edges, info.components, info.rounds, info.excluded) == (0, 1, 0, 0)
    torch.cuda.synchronize()
    down = float(c["N"][0, 2]) > 0  # against (0, 0, -1): flipped
    assert comp[0] == 0 and (comp[1:] == -7).all() and int(flip[0]) == int(down) == info.flipped and (u == -7).all() and (w == -7.0).all()
    assert np.array_equal(normals[:3].cpu().numpy().view(np.uint32), (-c["N"][0] if down else c["N"][0]).view(np.uint32)) and (normals[3:] == -7.0).all()
    eng.close()


def test_too_many_candidates_are_refused():
    """4. n * (k + 1) >= 2^31: the candidates would not be counted in 31 bits.  The smallest such set at k = 64, built on the device."""
    import torch

    from owlraytracing_amd import _orient_lib
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _orient_lib.load()
    n = -(-(1 << 31) // 65)
    assert n * 65 >= (1 << 31) > (n - 1) * 65
    eng = TrueKNN(device=0)
    try:
        gen = torch.Generator(device=eng.device).manual_seed(7)
        eng.build(torch.rand((n, 3), dtype=torch.float32, device=eng.device, generator=gen))
        small = torch.full((16,), -7, dtype=torch.int32, device=eng.device)  # never read, never written: the call is refused first
        o = _orient_lib.OrientOptions()
        o.d_normals = o.d_flip = small.data_ptr()
        o.direction[2] = 1.0
        info = _orient_lib.OrientInfo()
        info.rounds = 98
        o.k = 64
        assert lib.tknnOrientNormals(eng._h, ctypes.byref(o), ctypes.byref(info), None) == UNSUPPORTED and "2^31" in lib.tknnLastError().decode()
        o.k = 65
        assert lib.tknnOrientNormals(eng._h, ctypes.byref(o), ctypes.byref(info), None) == ARG, "k out of range comes first"
        torch.cuda.synchronize()
        assert info.rounds == 98 and (small == -7).all()
    finally:
        eng.close()
