"""What tknnRadiusNms (include/owlknn_nms.h) refuses, one fault per row and in the header's order, and that a refused call writes
nothing, neither outputs nor info; max_rounds below the need ends the call with TKNN_E_STATE, the rounds reported."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import nms_spec as ns  # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3


def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _nms_lib
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _nms_lib.load()
    c, want = ns.case("straddle_scored"), ns.want("straddle_scored")
    n, B = len(c["P"]), c["num_batches"]
    eng = TrueKNN(device=0)
    dev = eng.device
    guard = 1024
    keep = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device=dev)
    cover = torch.full((n + guard,), -7, dtype=torch.int32, device=dev)
    counts = torch.full((B + guard,), -7, dtype=torch.int32, device=dev)
    scores = torch.from_numpy(np.ascontiguousarray(c["scores"])).to(dev)
    info = _nms_lib.RadiusNmsInfo()

    def call(handle=None, options=True, **kw):
        o = _nms_lib.RadiusNmsOptions()
        o.radius, o.flags, o.max_rounds = float(c["r"]), 0, 0
        o.d_scores, o.d_keep, o.d_cover, o.d_counts = scores.data_ptr(), keep.data_ptr(), cover.data_ptr(), counts.data_ptr()
        for name, v in kw.items():
            setattr(o, name, v)
        info.node_tests, info.bad_scores, info.rounds = 99, 98, 97
        rc = lib.tknnRadiusNms(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)
        assert rc == 0 or rc == STATE and info.rounds != 97 or (info.node_tests == 99 and info.bad_scores == 98 and info.rounds == 97), \
            "a refused call leaves the info alone"
        return rc

    def untouched():
        return bool((keep == 0xA5).all()) and bool((cover == -7).all()) and bool((counts == -7).all())

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnRadiusNms: "), t
        return t

    # 1. missing pointers, before the state
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(d_keep=None) == ARG and "d_keep" in text()
    assert call(d_keep=None, radius=0.0) == ARG and "d_keep" in text()
    # 2. not built, before any look at the values
    assert call() == STATE and "tknnBuild" in text() and info.rounds == 97
    assert call(radius=0.0) == STATE and call(radius=float("nan")) == STATE and call(flags=_nms_lib.NMS_BY_NAME) == STATE and call(flags=6) == STATE
    assert info.rounds == 97
    eng.build(c["P"], batch=c["batch"], num_batches=B)
    assert call(d_keep=None, radius=-1.0) == ARG and "d_keep" in text()
    # 3. the values: the radius, then scores with BY_NAME, then an unknown flag
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(radius=bad) == ARG and "radius" in text()
    assert call(radius=0.0, flags=_nms_lib.NMS_BY_NAME) == ARG and "radius" in text()
    assert call(flags=_nms_lib.NMS_BY_NAME) == ARG and "d_scores" in text() and "TKNN_NMS_BY_NAME" in text()
    assert call(flags=_nms_lib.NMS_BY_NAME | 2) == ARG and "d_scores" in text()
    assert call(flags=2) == ARG and "flag" in text()
    assert call(flags=0x80000000, d_scores=None) == ARG and "flag" in text()
    assert call(max_rounds=-1) == ARG and "max_rounds" in text()
    assert untouched(), "a refused call writes nothing"
    # the call itself; nothing is written behind the outputs
    assert call() == 0 and info.kept == want["counts"].sum() and info.eligible == want["eligible"] and info.bad_scores == 0
    assert info.rounds >= 1 and info.solve_ms >= info.rounds_ms > 0 and info.init_ms > 0 and info.cover_ms > 0 and info.node_tests > 0 and info.point_tests > 0
    assert np.array_equal(keep[:n].cpu().numpy(), want["keep"].astype(np.uint8)) and np.array_equal(cover[:n].cpu().numpy(), want["cover"])
    assert np.array_equal(counts[:B].cpu().numpy(), want["counts"])
    assert (keep[n:] == 0xA5).all() and (cover[n:] == -7).all() and (counts[B:] == -7).all()
    # d_cover = NULL and d_counts = NULL are accepted; BY_NAME without scores
    keep.fill_(0xA5), cover.fill_(-7), counts.fill_(-7)
    by_name = ns.brute(c["P"], c["r"], batch=c["batch"], num_batches=B, by_name=True)
    assert call(d_scores=None, d_cover=None, d_counts=None, flags=_nms_lib.NMS_BY_NAME) == 0 and info.kept == by_name["counts"].sum()
    assert np.array_equal(keep[:n].cpu().numpy(), by_name["keep"].astype(np.uint8)) and (cover == -7).all() and (counts == -7).all()
    eng.close()


def test_max_rounds_ends_the_call():
    import torch

    from owlraytracing_amd import _nms_lib
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _nms_lib.load()
    c, want = ns.case("line_scored"), ns.want("line_scored")
    n = len(c["P"])
    eng = TrueKNN(device=0)
    eng.build(c["P"])
    keep = torch.full((n,), 0xA5, dtype=torch.uint8, device=eng.device)
    cover = torch.full((n,), -7, dtype=torch.int32, device=eng.device)
    scores = torch.from_numpy(np.ascontiguousarray(c["scores"])).to(eng.device)
    o = _nms_lib.RadiusNmsOptions()
    o.radius, o.max_rounds = float(c["r"]), 1
    o.d_scores, o.d_keep, o.d_cover = scores.data_ptr(), keep.data_ptr(), cover.data_ptr()
    info = _nms_lib.RadiusNmsInfo()
    assert lib.tknnRadiusNms(eng._h, ctypes.byref(o), ctypes.byref(info), None) == STATE
    assert "max_rounds" in lib.tknnLastError().decode() and info.rounds == 1
    assert 0 < info.undecided < n and info.eligible == n and info.kept == 0 and info.rounds_ms > 0
    assert (keep == 0xA5).all() and (cover == -7).all(), "a call that ran out of rounds writes no output"
    o.max_rounds = 0
    assert lib.tknnRadiusNms(eng._h, ctypes.byref(o), ctypes.byref(info), None) == 0 and 1 < info.rounds <= ns.LINE_POINTS and info.undecided == 0
    assert np.array_equal(keep.cpu().numpy(), want["keep"].astype(np.uint8)) and np.array_equal(cover.cpu().numpy(), want["cover"])
    eng.close()


def test_the_wrapper_passes_the_codes_on():
    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    c = ns.case("straddle")
    eng = TrueKNN(device=0)
    with pytest.raises(TknnError) as err:
        eng.radius_nms(0.1)
    assert err.value.code == STATE and str(err.value).count("tknnRadiusNms") == 1
    eng.build(c["P"], batch=c["batch"])
    for r in (0.0, -3.0, float("nan")):
        with pytest.raises(TknnError) as err:
            eng.radius_nms(r)
        assert err.value.code == ARG and "radius" in str(err.value)
    with pytest.raises(TknnError) as err:
        eng.radius_nms(0.1, scores=np.zeros(len(c["P"]), np.float32), by_name=True)
    assert err.value.code == ARG
    eng.close()
