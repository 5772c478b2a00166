"""What tknnPeriodicKnn (include/owlknn_periodic.h) refuses, one fault per row and in the header's order, and that a refused call
writes nothing, neither rows nor info."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import periodic_spec as ps  # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = -1, -3, -5
FLT_MAX = float(np.finfo(np.float32).max)


def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _periodic_lib
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _periodic_lib.load()
    P, Q, lo, period = ps.uniform_case()
    k, m, n = 6, len(Q), len(P)
    want = ps.knn_rows(P, Q, k, lo, period)
    eng = TrueKNN(device=0)
    dev = eng.device
    q = torch.from_numpy(np.array(Q)).to(dev)
    guard = 1024
    rows = max(m, n)
    idx = torch.full((rows * k + guard,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((rows * k + guard,), -7.0, dtype=torch.float32, device=dev)
    counts = torch.full((rows + guard,), -7, dtype=torch.int32, device=dev)
    skips = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    radii = torch.full((rows,), float("nan"), dtype=torch.float32, device=dev)
    info = _periodic_lib.PeriodicKnnInfo()

    def call(handle=None, options=True, **kw):
        o = _periodic_lib.PeriodicKnnOptions()
        o.d_queries, o.m, o.k, o.radius = q.data_ptr(), m, k, FLT_MAX
        o.lo, o.period = (ctypes.c_float * 3)(*[float(v) for v in lo]), (ctypes.c_float * 3)(*[float(v) for v in period])
        o.d_idx, o.d_dist, o.d_counts = idx.data_ptr(), dist.data_ptr(), counts.data_ptr()
        for name, v in kw.items():
            setattr(o, name, (ctypes.c_float * 3)(*[float(x) for x in v]) if name in ("lo", "period") else v)
        info.node_tests = 99
        rc = lib.tknnPeriodicKnn(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)
        assert rc == 0 or info.node_tests == 99, "a refused call leaves the info alone"
        return rc

    def untouched():
        return bool((idx == -7).all()) and bool((dist == -7.0).all()) and bool((counts == -7).all())

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnPeriodicKnn: "), t
        return t

    def axis(a, value, base):
        v = [float(x) for x in base]
        v[a] = value
        return v

    nan, inf = float("nan"), float("inf")
    # 1. missing pointers and the shape of a self-mode call, before the state
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(d_idx=None) == ARG and "d_idx" in text()
    assert call(d_idx=None, k=0, m=-1, period=(nan, 0, 0)) == ARG and "d_idx" in text()
    assert call(d_queries=None) == ARG and "m must equal n" in text(), "no tree: n = 0"
    assert call(d_queries=None, m=0, d_skip_ids=skips.data_ptr()) == ARG and "d_skip_ids" in text()
    # 2. not built, before any look at the values
    assert call() == STATE and "tknnBuild" in text()
    assert call(k=0) == STATE and call(m=-1) == STATE and call(k=65) == STATE and call(period=(nan, 0, 0)) == STATE and call(radius=0.0) == STATE
    eng.build(P)
    # 1. again, with a tree: self mode needs m = n and no skips
    for bad_m in (m, n - 1, n + 1, 0, -1):
        assert call(d_queries=None, m=bad_m) == ARG and "m must equal n" in text()
    assert call(d_queries=None, m=n, d_skip_ids=skips.data_ptr()) == ARG and "d_skip_ids" in text()
    assert call(d_queries=None, m=n, d_skip_ids=skips.data_ptr(), k=65) == ARG
    # 3. k and m
    assert call(k=0) == ARG and "k must be positive" in text()
    assert call(k=-3) == ARG and call(k=0, m=-1) == ARG and "k must be positive" in text()
    assert call(m=-1) == ARG and "2^31" in text() and call(m=2**31 - 1) == ARG and "2^31" in text()
    assert call(m=-1, k=65) == ARG, "m before the k above the register lists"
    # 4. k above the register lists, before the cell and the radius
    assert call(k=65) == UNSUPPORTED and "k out of range" in text()
    assert call(k=65, period=(nan, 0, 0), radius=-1.0) == UNSUPPORTED
    assert call(d_queries=None, m=n, k=65) == UNSUPPORTED
    # 5. the cell and the radius
    for a, name in enumerate("xyz"):
        for bad in (nan, -0.5, inf, -inf):
            assert call(period=axis(a, bad, period)) == ARG and "period" in text() and ("axis " + name) in text(), (name, bad)
    for a, name in enumerate("xy"):
        for bad in (nan, inf, -inf):
            assert call(lo=axis(a, bad, lo)) == ARG and "lo" in text() and ("axis " + name) in text(), (name, bad)
    assert call(lo=axis(2, nan, lo)) == 0, "lo of an open axis is not read"
    idx.fill_(-7), dist.fill_(-7.0), counts.fill_(-7)
    for bad in (nan, 0.0, -1.0, inf, -inf):
        assert call(radius=bad) == ARG and "radius" in text(), bad
    assert call(radius=nan, period=(nan, 0, 0)) == ARG and "period" in text(), "the cell before the radius"
    assert call(radius=nan, d_radii=radii.data_ptr()) == 0 and info.total == 0, "with d_radii the radius is not read; NaN radii: empty rows"
    assert bool((counts[:m] == 0).all()) and bool((idx[:m * k] == -1).all())
    idx.fill_(-7), dist.fill_(-7.0), counts.fill_(-7)
    # 6. the built set against the cell, after everything else
    assert call(lo=axis(0, float(lo[0]) + 0.01, lo)) == ARG and "axis x" in text() and "cell" in text()
    assert call(period=axis(1, 0.5, period)) == ARG and "axis y" in text()
    assert call(period=axis(2, 0.1, period), lo=axis(2, 0.0, lo)) == ARG and "axis z" in text(), "z is open in the case; as a periodic axis the set is outside"
    assert call(period=axis(1, 0.5, period), radius=nan) == ARG and "radius" in text(), "the radius before the set"
    assert untouched(), "a refused call writes nothing"
    # m = 0 with queries given: a zeroed info
    assert call(m=0) == 0 and info.node_tests == 0 and info.total == 0 and info.solve_ms == 0 and untouched()
    # the call itself; nothing is written behind the rows
    assert call() == 0 and info.total == want["counts"].sum() and info.full_rows == (want["counts"] == k).sum()
    assert info.solve_ms >= info.walk_ms > 0 and info.order_ms > 0 and info.seed_ms > 0 and info.node_tests > 0 and info.lane_rows == 0
    assert info.seed_point_tests == 32 * m, "two blocks of 16 around every query for k = 6"
    assert np.array_equal(idx[:m * k].view(m, k).cpu().numpy(), want["idx"]) and np.array_equal(counts[:m].cpu().numpy(), want["counts"])
    assert np.array_equal(dist[:m * k].view(m, k).cpu().numpy().view(np.int32), want["dist"].view(np.int32))
    assert (idx[m * k:] == -7).all() and (dist[m * k:] == -7.0).all() and (counts[m:] == -7).all()
    # d_dist = NULL and d_counts = NULL are accepted; negative skip ids skip nothing
    idx.fill_(-7), dist.fill_(-7.0), counts.fill_(-7)
    assert call(d_dist=None, d_counts=None, d_skip_ids=skips.data_ptr()) == 0 and info.total == want["counts"].sum()
    assert np.array_equal(idx[:m * k].view(m, k).cpu().numpy(), want["idx"]) and (dist == -7.0).all() and (counts == -7).all()
    # self mode through ctypes
    idx.fill_(-7)
    own = ps.self_rows(P, k, lo, period)
    assert call(d_queries=None, m=n) == 0 and info.total == own["counts"].sum()
    assert np.array_equal(idx[:n * k].view(n, k).cpu().numpy(), own["idx"]) and np.array_equal(counts[:n].cpu().numpy(), own["counts"])
    assert (idx[n * k:] == -7).all() and (counts[n:] == -7).all()
    eng.close()


def test_a_set_with_one_point_outside_the_cell_is_refused():
    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    P, Q, lo, period = ps.uniform_case()
    hi = (lo + period).astype(np.float32)
    for a, value in ((0, np.nextafter(lo[0], np.float32(-9))), (1, np.nextafter(np.nextafter(hi[1], np.float32(9)), np.float32(9))), (0, np.float32(0.5))):
        bad = np.array(P)
        bad[1234, a] = value
        assert not ps.in_cell(bad, lo, period).all()
        eng = TrueKNN(device=0)
        eng.build(bad)
        for kw in ({"queries": Q}, {}, {"queries": Q, "radius": 0.05}):
            with pytest.raises(TknnError) as err:
                eng.periodic_knn(k=5, lo=lo, period=period, **kw)
            assert err.value.code == ARG and "tknnPeriodicKnn: " in str(err.value) and ("axis " + "xy"[a]) in str(err.value)
        assert eng.periodic_knn(Q, 5, lo=lo, period=(0, 0, 0))["info"]["total"] == 5 * len(Q), "open axes take any set"
        if a == 0:
            assert eng.periodic_knn(Q, 5, lo=lo, period=(0, period[1], 0))["info"]["total"] > 0, "the other axis alone is fine"
        eng.close()
    # a NaN point is ignored by the box of the set
    nan = np.array(P)
    nan[7] = np.nan
    eng = TrueKNN(device=0)
    eng.build(nan)
    got = eng.periodic_knn(Q, 5, lo=lo, period=period)
    assert got["info"]["total"] == 5 * len(Q) and not (got["idx"] == 7).any()
    eng.close()


def test_the_wrapper_passes_the_codes_on():
    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    P, Q, lo, period = ps.uniform_case()
    eng = TrueKNN(device=0)
    with pytest.raises(TknnError) as err:
        eng.periodic_knn(Q, 5, lo=lo, period=period)
    assert err.value.code == STATE
    eng.build(P)
    for k, code in ((0, ARG), (-1, ARG), (65, UNSUPPORTED)):
        for kw in ({"queries": Q}, {}):
            with pytest.raises(TknnError) as err:
                eng.periodic_knn(k=k, lo=lo, period=period, **kw)
            assert err.value.code == code and str(err.value).count("tknnPeriodicKnn") == 1
    for kw in ({"radius": 0.0}, {"radius": float("inf")}, {"period": (-1, 0, 0)}, {"period": (float("nan"), 1, 1)}):
        with pytest.raises(TknnError) as err:
            eng.periodic_knn(Q, 5, **dict({"lo": lo, "period": period}, **kw))
        assert err.value.code == ARG
    eng.close()
