"""What tknnEmst (include/owlknn_emst.h) refuses, one fault per row and in the header's order, and that a refused call writes
nothing; then the argument checks of TrueKNN.emst above it."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import emst_spec as em  # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, ROUNDS = -1, -3, -4


def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _emst_lib
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _emst_lib.load()
    P, _, _, want = em.case("lattice")
    n = len(P)
    eng = TrueKNN(device=0)
    dev = eng.device
    guard = 1024
    u = torch.full((n - 1 + guard,), -7, dtype=torch.int32, device=dev)
    v = torch.full((n - 1 + guard,), -7, dtype=torch.int32, device=dev)
    w = torch.full((n - 1 + guard,), -7.0, dtype=torch.float32, device=dev)
    comp = torch.full((n + guard,), -7, dtype=torch.int32, device=dev)
    info = _emst_lib.EmstInfo()

    def call(handle=None, options=True, **kw):
        o = _emst_lib.EmstOptions()
        o.d_u, o.d_v, o.d_w, o.d_component = u.data_ptr(), v.data_ptr(), w.data_ptr(), comp.data_ptr()
        for name, value in kw.items():
            setattr(o, name, value)
        return lib.tknnEmst(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)

    def untouched():
        return bool((u == -7).all()) and bool((v == -7).all()) and bool((w == -7.0).all()) and bool((comp == -7).all())

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnEmst: "), t
        return t

    info.edges = 99
    # 1. missing engine and options, before the state
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    # 3. not built (no tree: n = 0, no pointer is asked for yet)
    assert call() == STATE and "tknnBuild" in text()
    assert call(d_u=None) == STATE and call(d_v=None, max_rounds=1) == STATE
    eng.build(P)
    # 2. d_u and d_v with n > 1
    assert call(d_u=None) == ARG and "d_u" in text()
    assert call(d_v=None) == ARG and "d_v" in text()
    assert call(d_u=None, d_v=None, max_rounds=1) == ARG and "d_u" in text()
    assert info.edges == 99, "a refused call leaves info alone"
    # 5. the round guard: nothing is written, info says how far the rounds came
    assert call(max_rounds=1) == ROUNDS and "max_rounds" in text()
    assert info.rounds == 1 and 0 < info.edges < n - 1 and info.components == n - info.edges
    assert untouched(), "a refused call writes nothing"
    # the call itself; nothing is written behind the rows
    assert call() == 0 and info.edges == want["edges"] == n - 1 and info.components == 1 and info.excluded == 0
    assert 2 <= info.rounds <= em.round_bound(n) and info.solve_ms >= info.walk_ms > 0 and info.node_tests > 0 and info.point_tests > 0
    assert np.array_equal(u[:n - 1].cpu().numpy(), want["u"]) and np.array_equal(v[:n - 1].cpu().numpy(), want["v"])
    assert np.array_equal(w[:n - 1].cpu().numpy().view(np.uint32), want["w"].view(np.uint32))
    assert np.array_equal(comp[:n].cpu().numpy(), want["component"])
    assert (u[n - 1:] == -7).all() and (v[n - 1:] == -7).all() and (w[n - 1:] == -7.0).all() and (comp[n:] == -7).all()
    # d_w = NULL and d_component = NULL are accepted
    u.fill_(-7), v.fill_(-7), w.fill_(-7.0), comp.fill_(-7)
    assert call(d_w=None, d_component=None) == 0 and info.edges == n - 1
    assert np.array_equal(u[:n - 1].cpu().numpy(), want["u"]) and (w == -7.0).all() and (comp == -7).all()
    # n = 1: d_u and d_v may be NULL
    eng.build(P[:1])
    comp.fill_(-7)
    assert call(d_u=None, d_v=None, d_w=None) == 0 and info.edges == 0 and info.components == 1 and info.rounds == 0
    assert comp[0] == 0 and (comp[1:] == -7).all()
    eng.close()


def test_the_wrapper_checks_its_arguments():
    import torch

    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    P = em.case("lattice")[0]
    n = len(P)
    eng = TrueKNN(device=0)
    with pytest.raises(TknnError) as err:
        eng.emst()
    assert err.value.code == STATE and str(err.value).count("tknnEmst") == 1
    eng.build(P)
    core = torch.zeros(n, dtype=torch.float32)
    for bad in (core, core.cuda().double(), core.cuda()[:-1], torch.zeros(2 * n, dtype=torch.float32).cuda()[::2], [0.0] * n,
                np.zeros(n - 1, np.float32), np.zeros((n, 1), np.float32)):
        with pytest.raises(ValueError):
            eng.emst(core_dist=bad)
    got = eng.emst(core_dist=np.zeros(n, np.float64))  # (numpy is converted)
    assert got["edges"] == n - 1 and "components" not in got
    eng.close()
