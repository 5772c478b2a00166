"""What tknnFps (include/owlknn_fps.h) refuses, one fault per row and in the header's order, and that a refused call writes
nothing, neither rows nor info."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import fps_spec as fs  # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3


def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _fps_lib
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _fps_lib.load()
    P, batch = fs.straddle_case()
    B, S = len(fs.STRADDLE_SIZES), 12
    want = fs.brute(P, S, batch=batch, num_batches=B)
    eng = TrueKNN(device=0)
    dev = eng.device
    guard = 1024
    idx = torch.full((B * S + guard,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((B * S + guard,), -7.0, dtype=torch.float32, device=dev)
    counts = torch.full((B + guard,), -7, dtype=torch.int32, device=dev)
    info = _fps_lib.FpsInfo()

    def call(handle=None, options=True, **kw):
        o = _fps_lib.FpsOptions()
        o.num_samples, o.flags = S, 0
        o.d_idx, o.d_dist, o.d_counts = idx.data_ptr(), dist.data_ptr(), counts.data_ptr()
        for name, v in kw.items():
            setattr(o, name, v)
        info.node_tests, info.bad_starts = 99, 98
        rc = lib.tknnFps(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)
        assert rc == 0 or (info.node_tests == 99 and info.bad_starts == 98), "a refused call leaves the info alone"
        return rc

    def untouched():
        return bool((idx == -7).all()) and bool((dist == -7.0).all()) and bool((counts == -7).all())

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnFps: "), t
        return t

    # 1. missing pointers, before the state
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(d_idx=None) == ARG and "d_idx" in text()
    assert call(d_idx=None, num_samples=0) == ARG and "d_idx" in text()
    # 2. not built, before any look at the values
    assert call() == STATE and "tknnBuild" in text()
    assert call(num_samples=0) == STATE and call(num_samples=-1) == STATE and call(num_samples=2**31 - 1) == STATE
    eng.build(P, batch=batch)
    assert call(d_idx=None, num_samples=0) == ARG and "d_idx" in text()
    # 3. the number of samples
    for bad in (0, -1, -2**31):
        assert call(num_samples=bad) == ARG and "num_samples" in text()
    big = (2**31 + B - 1) // B  # the first S with B * S >= 2^31
    assert call(num_samples=big) == ARG and "2^31" in text()
    assert call(num_samples=2**31 - 1) == ARG and "2^31" in text()
    assert untouched(), "a refused call writes nothing"
    # the call itself; nothing is written behind the rows
    assert call() == 0 and info.samples == want["counts"].sum() and info.bad_starts == 0 and info.lds_clouds == 0
    assert info.solve_ms >= info.walk_ms > 0 and info.init_ms > 0 and info.node_tests > 0 and info.point_tests > 0
    assert np.array_equal(idx[:B * S].view(B, S).cpu().numpy(), want["idx"]) and np.array_equal(counts[:B].cpu().numpy(), want["counts"])
    assert np.array_equal(dist[:B * S].view(B, S).cpu().numpy().view(np.int32), want["dist"].view(np.int32))
    assert (idx[B * S:] == -7).all() and (dist[B * S:] == -7.0).all() and (counts[B:] == -7).all()
    # d_dist = NULL and d_counts = NULL are accepted
    idx.fill_(-7), dist.fill_(-7.0), counts.fill_(-7)
    assert call(d_dist=None, d_counts=None, flags=_fps_lib.FPS_NO_PRUNE) == 0 and info.samples == want["counts"].sum()
    assert np.array_equal(idx[:B * S].view(B, S).cpu().numpy(), want["idx"]) and (dist == -7.0).all() and (counts == -7).all()
    # a plain tree is one cloud: B * S < 2^31 holds for every S
    eng.build(P)
    idx.fill_(-7)
    assert call(num_samples=3, d_dist=None, d_counts=None) == 0 and info.samples == 3
    assert idx[:3].cpu().numpy().tolist() == fs.brute(P, 3)["idx"][0].tolist() and (idx[3:] == -7).all()
    eng.close()


def test_the_wrapper_passes_the_codes_on():
    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    P, batch = fs.straddle_case()
    eng = TrueKNN(device=0)
    with pytest.raises(TknnError) as err:
        eng.fps(num_samples=4)
    assert err.value.code == STATE and str(err.value).count("tknnFps") == 1
    eng.build(P, batch=batch)
    for S in (0, -3):
        with pytest.raises(TknnError) as err:
            eng.fps(num_samples=S)
        assert err.value.code == ARG and "num_samples" in str(err.value)
    eng.close()
