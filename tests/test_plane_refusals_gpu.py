"""What tknnSegmentPlane (include/owlknn_plane.h) refuses, one fault per row and in the header's order, each said in the call's name
through tknnLastError, and that a refused call writes nothing, info included.  (No call of the library builds a box tree in an
engine: that refusal -- TKNN_E_STATE -- is not reached here.)"""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_spec as ps  # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = -1, -3, -5


def test_error_codes_in_order():
    import re

    import torch

    from owlraytracing_amd import _plane_lib
    from owlraytracing_amd.trueknn import TrueKNN

    with open(os.path.join(ROOT, "include", "owlknn.h")) as f:
        text = f.read()
    for name, code in (("TKNN_E_ARG", ARG), ("TKNN_E_UNSUPPORTED", UNSUPPORTED), ("TKNN_E_STATE", STATE)):
        assert int(re.search(r"%s = (-\d+)" % name, text).group(1)) == code, name
    lib = _plane_lib.load()
    c, want = ps.case("lattice")
    P, n, trials = c["P"], len(c["P"]), 64
    eng = TrueKNN(device=0)
    dev = eng.device
    guard = 1024
    mask = torch.full((n + guard,), 249, dtype=torch.uint8, device=dev)
    rows = torch.full((n + guard,), -7, dtype=torch.int32, device=dev)
    status = torch.full((trials + guard,), -7, dtype=torch.int32, device=dev)
    inliers = torch.full((trials + guard,), -7, dtype=torch.int32, device=dev)
    active = torch.ones((n,), dtype=torch.uint8, device=dev)
    info = _plane_lib.PlaneInfo()

    def call(handle=None, options=True, with_info=True, axis=(0, 0, 0), **kw):
        o = _plane_lib.PlaneOptions()
        o.d_active = active.data_ptr()
        o.distance_threshold, o.max_trials, o.confidence, o.seed, o.refit_rounds, o.min_cos = c["thr"], trials, 1.0, c["seed"], 1, 0.5
        o.d_inlier_mask, o.d_inlier_rows, o.d_trial_status, o.d_trial_inliers = mask.data_ptr(), rows.data_ptr(), status.data_ptr(), inliers.data_ptr()
        for i in range(3):
            o.axis[i] = axis[i]
        for name, value in kw.items():
            setattr(o, name, value)
        return lib.tknnSegmentPlane(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info) if with_info else None, None)

    def untouched():
        torch.cuda.synchronize()
        return bool((mask == 249).all()) and bool((rows == -7).all()) and bool((status == -7).all()) and bool((inliers == -7).all()) and bool((active == 1).all())

    def said():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnSegmentPlane: "), t
        return t

    info.inliers, info.best_trial, info.trials_run = 99, 98, 97
    nan, inf = float("nan"), float("inf")
    # 1. engine, options, info: before the state
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in said()
    assert call(options=False) == ARG and "options" in said()
    assert call(with_info=False) == ARG and "info" in said()
    # 2. not built, before the values
    assert call() == STATE and "tknnBuild" in said()
    assert call(distance_threshold=0.0) == STATE and call(max_trials=0) == STATE and call(flags=1) == STATE
    eng.build(P, ids=np.arange(n, dtype=np.int32) + 5)
    assert call() == UNSUPPORTED and "ids" in said()
    assert call(distance_threshold=-1.0) == UNSUPPORTED, "the tree before the values"
    eng.build(P)
    # 3. the values, in the header's order
    for bad in (0.0, -1.0, nan, inf):
        assert call(distance_threshold=bad) == ARG and "distance_threshold" in said()
    assert call(max_trials=0) == ARG and "max_trials" in said()
    assert call(max_trials=-5) == ARG
    for bad in (0.0, -0.5, 1.5, nan):
        assert call(confidence=bad) == ARG and "confidence" in said()
    for bad in (-1, 9):
        assert call(refit_rounds=bad) == ARG and "refit_rounds" in said()
    for bad in ((nan, 0, 1), (0, inf, 1), (0, 0, -inf)):
        assert call(axis=bad) == ARG and "axis" in said()
    for bad in (0.0, -0.5, 1.5, nan):
        assert call(axis=(0, 0, 1), min_cos=bad) == ARG and "min_cos" in said()
    assert call(flags=1) == ARG and "flags" in said()
    assert call(flags=0x80000000) == ARG
    # the order: each fault before the ones listed after it
    assert call(distance_threshold=0.0, max_trials=0) == ARG and "distance_threshold" in said()
    assert call(max_trials=0, confidence=2.0) == ARG and "max_trials" in said()
    assert call(confidence=2.0, refit_rounds=9) == ARG and "confidence" in said()
    assert call(refit_rounds=9, axis=(nan, 0, 0)) == ARG and "refit_rounds" in said()
    assert call(axis=(nan, 0, 1), min_cos=2.0) == ARG and "axis" in said()
    assert call(axis=(0, 0, 1), min_cos=2.0, flags=1) == ARG and "min_cos" in said()
    assert (info.inliers, info.best_trial, info.trials_run) == (99, 98, 97), "a refused call leaves info alone"
    assert untouched(), "a refused call writes nothing"
    # the call itself, with its options at their edges
    assert call(min_cos=7.0) == 0, "min_cos is not read without an axis"
    assert info.trials_run == trials and info.active == n and info.best_trial >= 0
    assert call(axis=(0, 0, 1), min_cos=1.0, refit_rounds=8, confidence=1e-9, max_trials=1) == 0 and info.trials_run == 1
    assert call(refit_rounds=0, d_inlier_mask=None, d_inlier_rows=None, d_trial_status=None, d_trial_inliers=None, d_active=None) == 0
    eng.close()
