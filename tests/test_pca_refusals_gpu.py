"""What tknnLocalPca (include/owlknn_pca.h) refuses, one fault per row and in the header's order, that the message names the field,
and that a refused call writes nothing, neither outputs nor info; and what an accepted call leaves alone: the cells behind its m
rows, and every buffer it was not asked for."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import pca_spec as ps  # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = -1, -3, -5


def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _pca_lib as pl
    from owlraytracing_amd.trueknn import TrueKNN

    lib = pl.load()
    c = ps.case("cube1025")
    n, m, guard = len(c["P"]), len(c["Q"]), 1024
    hood = c["hoods"][0]
    r = float(hood[1])
    eng = TrueKNN(device=0)
    dev = eng.device
    rows = max(n, m) + guard
    bufs = {name: torch.full((rows * width,), -7, dtype=torch.int32 if name == "counts" else torch.float32, device=dev) for name, (_, width) in pl.OUTPUTS.items()}
    Q = torch.from_numpy(np.array(c["Q"])).to(dev)
    info = pl.LocalPcaInfo()

    def call(handle=None, options=True, outputs=tuple(pl.OUTPUTS), viewpoint=None, **kw):
        o = pl.LocalPcaOptions()
        o.m, o.radius, o.k, o.min_points, o.flags = m, r, 0, 0, 0
        o.d_queries = Q.data_ptr()
        for name in outputs:
            setattr(o, pl.OUTPUTS[name][0], bufs[name].data_ptr())
        if viewpoint is not None:
            o.viewpoint[0], o.viewpoint[1], o.viewpoint[2] = viewpoint
        for name, v in kw.items():
            setattr(o, name, v)
        info.total, info.node_tests, info.walk_ms = 99, 98, 97.0
        rc = lib.tknnLocalPca(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)
        assert rc == 0 or (info.total == 99 and info.node_tests == 98 and info.walk_ms == 97.0), "a refused call leaves the info alone"
        return rc

    def untouched(but=()):
        return all(bool((b == -7).all()) for name, b in bufs.items() if name not in but)

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnLocalPca: "), t
        return t

    own = dict(d_queries=None, m=n)
    # 1. missing pointers, no output, an inconsistent m -- before the state
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(outputs=()) == ARG and "no output" in text()
    assert call(outputs=(), radius=0.0) == ARG and "no output" in text()
    assert call(d_queries=None, m=5) == ARG and "m must equal n" in text()  # (no tree: n = 0)
    # 2. not built, before any look at the values
    assert call() == STATE and "tknnBuild" in text()
    for bad in (dict(radius=0.0), dict(radius=float("nan")), dict(k=-1), dict(k=65), dict(flags=8), dict(flags=pl.PCA_SKIP_SELF), dict(min_points=-1), dict(m=-1)):
        assert call(**bad) == STATE
    eng.build(c["P"])
    assert call(outputs=(), radius=-1.0) == ARG and "no output" in text()
    assert call(d_queries=None, m=n - 1, radius=-1.0) == ARG and "m must equal n" in text()
    assert call(d_queries=None, m=n + 1) == ARG and "m must equal n" in text()
    # 3. the values, in the header's order
    assert call(radius=0.0) == ARG and "radius" in text() and " k" in text()
    assert call(radius=0.0, k=0, flags=8) == ARG and "radius" in text()
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert call(radius=bad) == ARG and "radius" in text()
        assert call(radius=bad, k=5) == ARG and "radius" in text()
    assert call(radius=-1.0, k=-1) == ARG and "radius" in text()
    for bad in (-1, -100):
        assert call(k=bad) == ARG and "k must not be negative" in text()
    assert call(k=-1, flags=8) == ARG and "k must not be negative" in text()
    assert call(k=1, **own) == ARG and "k = 1" in text() and "TKNN_PCA_SKIP_SELF" in text()
    assert call(k=1, radius=0.0, **own) == ARG and "k = 1" in text()
    assert call(k=1, flags=8, **own) == ARG and "k = 1" in text()
    for bad in (4, 8, 0x80000000, pl.PCA_ORIENT | 16):
        assert call(flags=bad) == ARG and "flag" in text()
    assert call(flags=4 | pl.PCA_SKIP_SELF) == ARG and "flag" in text()
    assert call(flags=pl.PCA_SKIP_SELF) == ARG and "TKNN_PCA_SKIP_SELF" in text() and "d_queries" in text()
    assert call(flags=pl.PCA_SKIP_SELF | pl.PCA_ORIENT, viewpoint=(float("nan"), 0, 0)) == ARG and "TKNN_PCA_SKIP_SELF" in text()
    for bad in ((float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, -float("inf"))):
        assert call(flags=pl.PCA_ORIENT, viewpoint=bad) == ARG and "viewpoint" in text()
    assert call(viewpoint=(float("nan"), 0, 0)) == 0, "the viewpoint is read with TKNN_PCA_ORIENT only"
    for b in bufs.values():
        b.fill_(-7)
    assert call(flags=pl.PCA_ORIENT, viewpoint=(float("nan"), 0, 0), min_points=-1) == ARG and "viewpoint" in text()
    for bad in (-1, -50):
        assert call(min_points=bad) == ARG and "min_points" in text()
    assert call(min_points=-1, m=-1) == ARG and "min_points" in text()
    assert call(m=-1) == ARG and " m " in text()
    assert call(m=2 ** 31 - 1) == ARG and " m " in text()
    assert call(m=-1, k=65) == ARG and " m " in text()
    # 4. k above the register lists
    for bad in (65, 1000):
        assert call(k=bad) == UNSUPPORTED and "k out of range" in text()
        assert call(k=bad, radius=0.0) == UNSUPPORTED
    assert untouched(), "a refused call writes nothing"
    # 5. no queries: success, a zeroed info, nothing written
    assert call(m=0) == 0 and info.total == 0 and info.node_tests == 0 and info.walk_ms == 0 and untouched()
    # the call itself; nothing is written behind the outputs
    w = ps.want_of("cube1025", "ext", hood)[1]
    assert call() == 0 and info.total == w["len"].sum() and info.max_row == w["len"].max() and info.degenerate_rows == (~w["solved"]).sum()
    assert info.fallback_items == 0 and info.bound_ms == 0 and info.order_ms > 0 and info.solve_ms >= info.walk_ms > 0 and info.finish_ms > 0
    assert info.node_tests > 0 and info.point_tests > 0
    assert np.array_equal(bufs["counts"][:m].cpu().numpy(), w["counts"])
    for name, (_, width) in pl.OUTPUTS.items():
        assert (bufs[name][m * width:] == -7).all() and not (bufs[name][:m * width] == -7).any(), name
    everything = {name: b.clone() for name, b in bufs.items()}
    # every output asked alone: the same bits, and the buffers that were not asked for stay untouched
    for name, (_, width) in pl.OUTPUTS.items():
        for b in bufs.values():
            b.fill_(-7)
        assert call(outputs=(name,)) == 0 and untouched(but=(name,))
        assert torch.equal(bufs[name].view(torch.int32), everything[name].view(torch.int32)), name
    # the own points, with k and with the self left out, are accepted; k runs the bound
    for b in bufs.values():
        b.fill_(-7)
    assert call(flags=pl.PCA_SKIP_SELF, k=16, radius=0.0, **own) == 0 and info.order_ms == 0 and info.bound_ms > 0 and info.total == 16 * n
    assert call(flags=pl.PCA_SKIP_SELF, k=16, **own) == 0 and info.total == ps.want_of("cube1025", "own_skip", c["hoods"][-1])[1]["len"].sum()
    assert call(k=2, radius=0.0, **own) == 0 and info.total == 2 * n and info.degenerate_rows == n
    for name, (_, width) in pl.OUTPUTS.items():
        assert (bufs[name][n * width:] == -7).all(), name
    eng.close()


def test_the_wrapper_passes_the_codes_on():
    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    c = ps.case("cube15")
    eng = TrueKNN(device=0)
    with pytest.raises(TknnError) as err:
        eng.local_pca(radius=0.1, queries=c["Q"])
    assert err.value.code == STATE and str(err.value).count("tknnLocalPca") == 1
    eng.build(c["P"])
    with pytest.raises(TknnError) as err:
        eng.local_pca(queries=c["Q"])
    assert err.value.code == ARG and "radius" in str(err.value)
    for r in (-3.0, float("nan")):
        with pytest.raises(TknnError) as err:
            eng.local_pca(radius=r, queries=c["Q"])
        assert err.value.code == ARG and "radius" in str(err.value)
    with pytest.raises(TknnError) as err:
        eng.local_pca(radius=0.1, queries=c["Q"], skip_self=True)
    assert err.value.code == ARG and "TKNN_PCA_SKIP_SELF" in str(err.value)
    with pytest.raises(TknnError) as err:
        eng.local_pca(k=1)
    assert err.value.code == ARG and "k = 1" in str(err.value)
    with pytest.raises(TknnError) as err:
        eng.local_pca(k=65, queries=c["Q"])
    assert err.value.code == UNSUPPORTED
    with pytest.raises(TknnError) as err:
        eng.local_pca(radius=0.1, want=())
    assert err.value.code == ARG and "no output" in str(err.value)
    with pytest.raises(ValueError):
        eng.local_pca(radius=0.1, want=("normal",))
    with pytest.raises(ValueError):
        eng.local_pca(radius=0.1, viewpoint=(0, 0))
    eng.close()
