"""What tknnRadiusReduce (include/owlknn_reduce.h) refuses, one fault per row and in the header's order, that the message names
the field, and that a refused call writes nothing, neither outputs nor info."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import reduce_spec as rd  # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3


def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _reduce_lib as rl
    from owlraytracing_amd.trueknn import TrueKNN

    lib = rl.load()
    c = rd.case("n1025")
    n, m, C, guard = len(c["P"]), len(c["Q"]), 3, 1024
    r = c["radii"]["mid"]
    eng = TrueKNN(device=0)
    dev = eng.device
    rows = max(n, m) + guard
    counts = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    wsum = torch.full((rows,), -7.0, dtype=torch.float32, device=dev)
    out = torch.full((rows * C,), -7.0, dtype=torch.float32, device=dev)
    Q = torch.from_numpy(np.array(c["Q"])).to(dev)
    values = torch.from_numpy(np.ascontiguousarray(c["values"][:, :C])).to(dev)
    info = rl.RadiusReduceInfo()

    def call(handle=None, options=True, **kw):
        o = rl.RadiusReduceOptions()
        o.m, o.radius, o.bandwidth, o.weight, o.channels, o.flags = m, float(r), float(rd.bandwidth(r)), rl.W_GAUSS, C, 0
        o.d_queries, o.d_values = Q.data_ptr(), values.data_ptr()
        o.d_counts, o.d_wsum, o.d_out = counts.data_ptr(), wsum.data_ptr(), out.data_ptr()
        for name, v in kw.items():
            setattr(o, name, v)
        info.total, info.node_tests, info.walk_ms = 99, 98, 97.0
        rc = lib.tknnRadiusReduce(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)
        assert rc == 0 or (info.total == 99 and info.node_tests == 98 and info.walk_ms == 97.0), "a refused call leaves the info alone"
        return rc

    def untouched():
        return bool((counts == -7).all()) and bool((wsum == -7).all()) and bool((out == -7).all())

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnRadiusReduce: "), t
        return t

    own = dict(d_queries=None, m=n)
    # 1. missing pointers, no output, an inconsistent m -- before the state
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(d_counts=None, d_wsum=None, d_out=None) == ARG and "no output" in text()
    assert call(d_counts=None, d_wsum=None, d_out=None, radius=0.0) == ARG and "no output" in text()
    assert call(d_queries=None, m=5) == ARG and "m must equal n" in text()  # (no tree: n = 0)
    # 2. not built, before any look at the values
    assert call() == STATE and "tknnBuild" in text()
    for bad in (dict(radius=0.0), dict(radius=float("nan")), dict(weight=9), dict(flags=8), dict(channels=40), dict(flags=rl.REDUCE_SKIP_SELF), dict(m=-1)):
        assert call(**bad) == STATE
    eng.build(c["P"])
    assert call(d_counts=None, d_wsum=None, d_out=None, radius=-1.0) == ARG and "no output" in text()
    assert call(d_queries=None, m=n - 1, radius=-1.0) == ARG and "m must equal n" in text()
    assert call(d_queries=None, m=n + 1) == ARG and "m must equal n" in text()
    # 3. the values, in the header's order
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(radius=bad) == ARG and "radius" in text()
    assert call(radius=0.0, weight=9) == ARG and "radius" in text()
    for bad in (-1, 4, 100):
        assert call(weight=bad) == ARG and "weight" in text()
    assert call(weight=4, flags=4) == ARG and "weight" in text()
    for bad in (4, 8, 0x80000000, rl.REDUCE_NORMALIZE | 16):
        assert call(flags=bad) == ARG and "flag" in text()
    assert call(flags=4, bandwidth=0.0) == ARG and "flag" in text()
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        assert call(bandwidth=bad) == ARG and "bandwidth" in text()
    assert call(bandwidth=0.0, weight=rl.W_EPANECHNIKOV) == 0, "the bandwidth is read with the Gauss weight only"
    counts.fill_(-7), wsum.fill_(-7), out.fill_(-7)
    assert call(bandwidth=0.0, channels=17) == ARG and "bandwidth" in text()
    for bad in (-1, 17, 1 << 20):
        assert call(channels=bad) == ARG and "channels" in text()
    assert call(channels=17, d_values=None) == ARG and "channels" in text()
    assert call(d_values=None) == ARG and "d_values" in text()
    assert call(d_out=None) == ARG and "d_out" in text()
    assert call(d_values=None, d_out=None) == ARG and "d_values" in text()
    assert call(channels=0, d_counts=None, d_wsum=None) == ARG and "d_counts" in text()
    assert call(d_out=None, flags=rl.REDUCE_SKIP_SELF) == ARG and "d_out" in text()
    assert call(flags=rl.REDUCE_SKIP_SELF) == ARG and "TKNN_REDUCE_SKIP_SELF" in text() and "d_queries" in text()
    assert call(flags=rl.REDUCE_SKIP_SELF, m=-1) == ARG and "TKNN_REDUCE_SKIP_SELF" in text()
    assert call(m=-1) == ARG and " m " in text()
    assert call(m=2 ** 31 - 1) == ARG and " m " in text()
    assert untouched(), "a refused call writes nothing"
    # 4. no queries: success, a zeroed info, nothing written
    assert call(m=0) == 0 and info.total == 0 and info.node_tests == 0 and info.walk_ms == 0 and untouched()
    # the call itself; nothing is written behind the outputs
    want = rd.sums(rd.rows_of("n1025", "mid", "ext"), c["values"][:, :C], "gauss", r, rd.bandwidth(r))
    assert call() == 0 and info.total == want["counts"].sum() and info.max_row == want["counts"].max() and info.fallback_items == 0
    assert info.solve_ms >= info.walk_ms > 0 and info.order_ms > 0 and info.stage_ms > 0 and info.node_tests > 0 and info.point_tests > 0
    rd.compare({"counts": counts[:m].cpu().numpy(), "wsum": wsum[:m].cpu().numpy(), "out": out[:m * C].cpu().numpy().reshape(m, C)}, want, "gauss", r,
               rd.bandwidth(r), channels=C)
    assert (counts[m:] == -7).all() and (wsum[m:] == -7).all() and (out[m * C:] == -7).all()
    # the own points with the self left out are accepted
    assert call(flags=rl.REDUCE_SKIP_SELF, **own) == 0 and info.order_ms == 0
    assert (counts[n:] == -7).all() and (wsum[n:] == -7).all() and (out[n * C:] == -7).all()
    eng.close()


def test_the_wrapper_passes_the_codes_on():
    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    c = rd.case("n17")
    eng = TrueKNN(device=0)
    with pytest.raises(TknnError) as err:
        eng.radius_reduce(0.1, queries=c["Q"])
    assert err.value.code == STATE and str(err.value).count("tknnRadiusReduce") == 1
    eng.build(c["P"])
    for r in (0.0, -3.0, float("nan")):
        with pytest.raises(TknnError) as err:
            eng.radius_reduce(r, queries=c["Q"])
        assert err.value.code == ARG and "radius" in str(err.value)
    with pytest.raises(TknnError) as err:
        eng.radius_reduce(0.1, queries=c["Q"], skip_self=True)
    assert err.value.code == ARG and "TKNN_REDUCE_SKIP_SELF" in str(err.value)
    with pytest.raises(TknnError) as err:
        eng.radius_reduce(0.1, queries=c["Q"], weight="gauss", bandwidth=0.0)
    assert err.value.code == ARG and "bandwidth" in str(err.value)
    with pytest.raises(TknnError) as err:
        eng.radius_reduce(0.1, queries=c["Q"], want_wsum=False, want_counts=False)
    assert err.value.code == ARG and "no output" in str(err.value)
    eng.close()
