"""What tknnKnn (include/owlknn_knn.h) refuses, one fault per row and in the header's order, and that a refused call writes
nothing; then the argument checks of TrueKNN.knn above it."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_spec as kn  # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = -1, -3, -5


def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _knn_lib
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _knn_lib.load()
    P, Q = kn.lattice_case()
    k, m, n = 6, len(Q), len(P)
    want = kn.knn_rows(P, Q, k)
    eng = TrueKNN(device=0)
    dev = eng.device
    q = torch.from_numpy(np.array(Q)).to(dev)
    guard = 1024
    rows = max(m, n)
    idx = torch.full((rows * k + guard,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((rows * k + guard,), -7.0, dtype=torch.float32, device=dev)
    counts = torch.full((rows + guard,), -7, dtype=torch.int32, device=dev)
    skips = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    info = _knn_lib.KnnInfo()

    def call(handle=None, options=True, **kw):
        o = _knn_lib.KnnOptions()
        o.d_queries, o.m, o.k = q.data_ptr(), m, k
        o.d_idx, o.d_dist, o.d_counts = idx.data_ptr(), dist.data_ptr(), counts.data_ptr()
        for name, v in kw.items():
            setattr(o, name, v)
        return lib.tknnKnn(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)

    def untouched():
        return bool((idx == -7).all()) and bool((dist == -7.0).all()) and bool((counts == -7).all())

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnKnn: "), t
        return t

    # 1. missing pointers and the shape of a self-mode call, before the state
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(d_idx=None) == ARG and "d_idx" in text()
    assert call(d_idx=None, k=0, m=-1) == ARG and "d_idx" in text()
    assert call(d_queries=None) == ARG and "m must equal n" in text(), "no tree: n = 0"
    assert call(d_queries=None, m=0, d_skip_ids=skips.data_ptr()) == ARG and "d_skip_ids" in text()
    # 2. not built, before any look at the values
    assert call() == STATE and "tknnBuild" in text()
    assert call(k=0) == STATE and call(m=-1) == STATE and call(k=65) == STATE and call(d_queries=None, m=0) == STATE
    eng.build(P)
    # 1. again, with a tree: self mode needs m = n and no skips
    for bad_m in (m, n - 1, n + 1, 0, -1):
        assert call(d_queries=None, m=bad_m) == ARG and "m must equal n" in text()
    assert call(d_queries=None, m=n - 1, k=0) == ARG and "m must equal n" in text()
    assert call(d_queries=None, m=n, d_skip_ids=skips.data_ptr()) == ARG and "d_skip_ids" in text()
    assert call(d_queries=None, m=n, d_skip_ids=skips.data_ptr(), k=65) == ARG
    # 3. the values
    assert call(k=0) == ARG and "k must be positive" in text()
    assert call(k=-3) == ARG and call(k=0, m=-1) == ARG and "k must be positive" in text()
    assert call(m=-1) == ARG and "2^31" in text() and call(m=2**31 - 1) == ARG and "2^31" in text()
    assert call(m=-1, k=65) == ARG, "m before the k above the register lists"
    assert call(d_queries=None, m=n, k=0) == ARG and "k must be positive" in text()
    # 4. k above the register lists
    assert call(k=65) == UNSUPPORTED and "k out of range" in text()
    assert call(d_queries=None, m=n, k=65) == UNSUPPORTED
    assert untouched(), "a refused call writes nothing"
    # m = 0 with queries given: a zeroed info
    info.node_tests = 99
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
    own = kn.self_rows(P, k)
    assert call(d_queries=None, m=n) == 0 and info.total == own["counts"].sum()
    assert np.array_equal(idx[:n * k].view(n, k).cpu().numpy(), own["idx"]) and np.array_equal(counts[:n].cpu().numpy(), own["counts"])
    assert (idx[n * k:] == -7).all() and (counts[n:] == -7).all()
    eng.close()


def test_the_wrapper_checks_its_arguments():
    import torch

    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    P, Q = kn.lattice_case()
    eng = TrueKNN(device=0)
    with pytest.raises(TknnError) as err:
        eng.knn(Q, 5)
    assert err.value.code == STATE
    eng.build(P)
    tq = torch.from_numpy(np.array(Q))
    for bad in (Q.astype(np.float64)[:, :1], tq, tq.cuda().double(), tq.cuda()[:, :2], tq.cuda()[::2], [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError):
            eng.knn(bad, 5)
    with pytest.raises(ValueError):
        eng.knn(Q, 5, skip_ids=np.zeros(len(Q) - 1, np.int32))
    with pytest.raises(ValueError):
        eng.knn(Q, 5, skip_ids=torch.zeros(len(Q), dtype=torch.int32))  # on the host
    with pytest.raises(ValueError):
        eng.knn(k=5, skip_ids=np.zeros(len(P), np.int32))
    for k, code in ((0, ARG), (-1, ARG), (65, UNSUPPORTED)):
        for kw in ({"queries": Q}, {}):
            with pytest.raises(TknnError) as err:
                eng.knn(k=k, **kw)
            assert err.value.code == code and str(err.value).count("tknnKnn") == 1
    eng.close()
