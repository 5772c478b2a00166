"""What tknnBuildBatched, tknnBatchLayout and tknnBatchKnn (include/owlknn_batch.h) refuse, one fault per row and in the header's
order, and that a refused call writes nothing, neither rows nor info."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_spec as bs  # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = -1, -3, -5
FLT_MAX = float(np.finfo(np.float32).max)


def test_build_error_codes_in_order():
    import torch

    from owlraytracing_amd import _batch_lib, _lib
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _batch_lib.load()
    P, batch, Q, bq = bs.clouds_case()
    n, B = len(P), len(bs.CLOUD_SIZES)
    eng = TrueKNN(device=0)
    dev = eng.device
    xyz, labels = torch.from_numpy(np.array(P)).to(dev), torch.from_numpy(batch.copy()).to(dev)
    info = _lib.BuildInfo()

    def build(handle=None, d_xyz=xyz.data_ptr(), d_batch=labels.data_ptr(), num_batches=B, count=n):
        info.n = -99
        rc = lib.tknnBuildBatched(eng._h if handle is None else handle, d_xyz, None, d_batch, num_batches, count, ctypes.byref(info), None)
        assert rc == 0 or info.n == -99, "a refused build leaves the info alone"
        return rc

    def text(fn="tknnBuildBatched"):
        t = lib.tknnLastError().decode()
        assert t.startswith(fn + ": "), t
        return t

    def layout():
        nb, bits = ctypes.c_int32(-7), ctypes.c_int32(-7)
        rc = lib.tknnBatchLayout(eng._h, ctypes.byref(nb), ctypes.byref(bits), None, None)
        return rc, nb.value, bits.value

    # 1. missing pointers
    assert build(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert build(d_xyz=None) == ARG and "d_xyz" in text()
    assert build(d_batch=None) == ARG and "d_batch" in text()
    assert build(d_xyz=None, count=0, num_batches=0) == ARG and "d_xyz" in text()
    # 2. n, as tknnBuild refuses it
    for bad in (0, -1, 2**31 - 1):
        assert build(count=bad) == ARG and "n" in text()
        assert build(count=bad, num_batches=0) == ARG and "2^31" in text(), "n before num_batches"
    # 3. and 4. the number of batches
    for bad in (0, -1):
        assert build(num_batches=bad) == ARG and "num_batches" in text()
    assert build(num_batches=bs.MAX_BATCHES + 1) == UNSUPPORTED and "num_batches" in text()
    assert layout() == (STATE, -7, -7) and "tknnBuildBatched" in text("tknnBatchLayout"), "nothing has been built"
    # 5. a label outside [0, num_batches): the engine is left without a tree
    assert build() == 0 and info.n == n and layout() == (0, B, 3)
    assert build(num_batches=B - 1) == ARG and ("%d of the" % bs.CLOUD_SIZES[-1]) in text() and "labels" in text()
    assert layout()[0] == STATE
    with pytest.raises(_lib.TknnError) as err:
        eng.knn(Q, 3)
    assert err.value.code == STATE, "no tree after a refused batched build"
    labels[5] = -1
    assert build() == ARG and "1 of the" in text()
    labels[5] = int(batch[5])
    assert build(num_batches=bs.MAX_BATCHES) == 0 and layout() == (0, bs.MAX_BATCHES, 15)
    assert build() == 0 and layout() == (0, B, 3)
    # a plain rebuild forgets the batches
    eng.build(P)
    assert layout()[0] == STATE
    with pytest.raises(_lib.TknnError) as err:
        eng.batch_knn(Q, 3, batch=bq)
    assert err.value.code == STATE and "tknnBuildBatched" in str(err.value)
    with pytest.raises(_lib.TknnError) as err:
        eng.batch_layout()
    assert err.value.code == STATE
    eng.close()


def test_query_error_codes_in_order():
    import torch

    from owlraytracing_amd import _batch_lib
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _batch_lib.load()
    P, batch, Q, bq = bs.clouds_case()
    k, m, n = 6, len(Q), len(P)
    want = bs.knn_rows(P, batch, Q, bq, k)
    eng = TrueKNN(device=0)
    dev = eng.device
    q, qb = torch.from_numpy(np.array(Q)).to(dev), torch.from_numpy(bq.copy()).to(dev)
    guard = 1024
    rows = max(m, n)
    idx = torch.full((rows * k + guard,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((rows * k + guard,), -7.0, dtype=torch.float32, device=dev)
    counts = torch.full((rows + guard,), -7, dtype=torch.int32, device=dev)
    skips = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    radii = torch.full((rows,), float("nan"), dtype=torch.float32, device=dev)
    info = _batch_lib.BatchKnnInfo()

    def call(handle=None, options=True, **kw):
        o = _batch_lib.BatchKnnOptions()
        o.d_queries, o.d_query_batch, o.m, o.k, o.radius = q.data_ptr(), qb.data_ptr(), m, k, FLT_MAX
        o.d_idx, o.d_dist, o.d_counts = idx.data_ptr(), dist.data_ptr(), counts.data_ptr()
        for name, v in kw.items():
            setattr(o, name, v)
        info.node_tests = 99
        rc = lib.tknnBatchKnn(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)
        assert rc == 0 or info.node_tests == 99, "a refused call leaves the info alone"
        return rc

    def untouched():
        return bool((idx == -7).all()) and bool((dist == -7.0).all()) and bool((counts == -7).all())

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnBatchKnn: "), t
        return t

    own_mode = {"d_queries": None, "d_query_batch": None}
    nan, inf = float("nan"), float("inf")
    # 1. missing pointers and the shape of a self-mode call, before the state
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(d_idx=None) == ARG and "d_idx" in text()
    assert call(d_idx=None, k=0, m=-1, radius=nan) == ARG and "d_idx" in text()
    assert call(**own_mode) == ARG and "m must equal n" in text(), "no tree: n = 0"
    assert call(m=0, d_skip_ids=skips.data_ptr(), **own_mode) == ARG and "d_skip_ids" in text()
    assert call(d_query_batch=None) == ARG and "d_query_batch" in text()
    assert call(d_queries=None, m=0) == ARG and "d_query_batch" in text()
    # 2. not built, before any look at the values
    assert call() == STATE and "tknnBuildBatched" in text()
    assert call(k=0) == STATE and call(m=-1) == STATE and call(k=65) == STATE and call(radius=0.0) == STATE
    # 2. built without batches
    eng.build(P)
    assert call() == STATE and "tknnBuildBatched" in text() and call(k=0) == STATE and call(m=n, **own_mode) == STATE
    eng.build(P, batch=batch)
    # 1. again, with a tree: self mode needs m = n, no skips and no labels
    for bad_m in (m, n - 1, n + 1, 0, -1):
        assert call(m=bad_m, **own_mode) == ARG and "m must equal n" in text()
    assert call(m=n, d_skip_ids=skips.data_ptr(), **own_mode) == ARG and "d_skip_ids" in text()
    assert call(m=n, d_queries=None) == ARG and "d_query_batch" in text()
    assert call(d_query_batch=None, k=65) == ARG and "d_query_batch" in text()
    # 3. k and m
    assert call(k=0) == ARG and "k must be positive" in text()
    assert call(k=-3) == ARG and call(k=0, m=-1) == ARG and "k must be positive" in text()
    assert call(m=-1) == ARG and "2^31" in text() and call(m=2**31 - 1) == ARG and "2^31" in text()
    assert call(m=-1, k=65) == ARG, "m before the k above the register lists"
    # 4. k above the register lists, before the radius
    assert call(k=65) == UNSUPPORTED and "k out of range" in text()
    assert call(k=65, radius=-1.0) == UNSUPPORTED
    assert call(m=n, k=65, **own_mode) == UNSUPPORTED
    # 5. the radius
    for bad in (nan, 0.0, -1.0, inf, -inf):
        assert call(radius=bad) == ARG and "radius" in text(), bad
    assert untouched(), "a refused call writes nothing"
    assert call(radius=nan, d_radii=radii.data_ptr()) == 0 and info.total == 0, "with d_radii the radius is not read; NaN radii: empty rows"
    assert bool((counts[:m] == 0).all()) and bool((idx[:m * k] == -1).all())
    idx.fill_(-7), dist.fill_(-7.0), counts.fill_(-7)
    # m = 0 with queries given: a zeroed info
    assert call(m=0) == 0 and info.node_tests == 0 and info.total == 0 and info.solve_ms == 0 and untouched()
    # the call itself; nothing is written behind the rows
    assert call() == 0 and info.total == want["counts"].sum() and info.full_rows == (want["counts"] == k).sum()
    assert info.solve_ms >= info.walk_ms > 0 and info.order_ms > 0 and info.seed_ms > 0 and info.node_tests > 0 and info.lane_rows == 0
    assert 0 < info.seed_point_tests <= 32 * m, "at most two blocks of 16 around every query for k = 6"
    assert np.array_equal(idx[:m * k].view(m, k).cpu().numpy(), want["idx"]) and np.array_equal(counts[:m].cpu().numpy(), want["counts"])
    assert np.array_equal(dist[:m * k].view(m, k).cpu().numpy().view(np.int32), want["dist"].view(np.int32))
    assert (idx[m * k:] == -7).all() and (dist[m * k:] == -7.0).all() and (counts[m:] == -7).all()
    # d_dist = NULL and d_counts = NULL are accepted; negative skip ids skip nothing
    idx.fill_(-7), dist.fill_(-7.0), counts.fill_(-7)
    assert call(d_dist=None, d_counts=None, d_skip_ids=skips.data_ptr()) == 0 and info.total == want["counts"].sum()
    assert np.array_equal(idx[:m * k].view(m, k).cpu().numpy(), want["idx"]) and (dist == -7.0).all() and (counts == -7).all()
    # self mode through ctypes
    idx.fill_(-7)
    own = bs.self_rows(P, batch, k)
    assert call(m=n, **own_mode) == 0 and info.total == own["counts"].sum()
    assert np.array_equal(idx[:n * k].view(n, k).cpu().numpy(), own["idx"]) and np.array_equal(counts[:n].cpu().numpy(), own["counts"])
    assert (idx[n * k:] == -7).all() and (counts[n:] == -7).all()
    # the layout's starts, on the device
    starts = torch.full((len(bs.CLOUD_SIZES) + 1 + guard,), -7, dtype=torch.int32, device=dev)
    assert lib.tknnBatchLayout(eng._h, None, None, starts.data_ptr(), None) == 0
    assert starts[:len(bs.CLOUD_SIZES) + 1].cpu().numpy().tolist() == np.concatenate([[0], np.cumsum(bs.CLOUD_SIZES)]).tolist()
    assert (starts[len(bs.CLOUD_SIZES) + 1:] == -7).all()
    eng.close()


def test_the_wrapper_passes_the_codes_on():
    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    P, batch, Q, bq = bs.clouds_case()
    eng = TrueKNN(device=0)
    with pytest.raises(TknnError) as err:
        eng.batch_knn(Q, 5, batch=bq)
    assert err.value.code == STATE
    with pytest.raises(TknnError) as err:
        eng.build(P, batch=batch, num_batches=3)
    assert err.value.code == ARG and str(err.value).count("tknnBuildBatched") == 1
    with pytest.raises(TknnError) as err:
        eng.build(P, batch=batch, num_batches=bs.MAX_BATCHES + 1)
    assert err.value.code == UNSUPPORTED
    eng.build(P, batch=batch)
    for k, code in ((0, ARG), (-1, ARG), (65, UNSUPPORTED)):
        for kw in ({"queries": Q, "batch": bq}, {}):
            with pytest.raises(TknnError) as err:
                eng.batch_knn(k=k, **kw)
            assert err.value.code == code and str(err.value).count("tknnBatchKnn") == 1
    for radius in (0.0, float("inf"), float("nan")):
        with pytest.raises(TknnError) as err:
            eng.batch_knn(Q, 5, batch=bq, radius=radius)
        assert err.value.code == ARG
    eng.close()
