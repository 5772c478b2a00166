"""What tknnIcp (include/owlknn_icp.h) refuses, one fault per row and in the header's order, that the message names the field, and
that a refused call writes nothing, neither outputs nor info; the trees it does not take; and what an accepted call leaves alone."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = -1, -3, -5
NAN, INF = float("nan"), float("inf")


def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _icp_lib as il
    from owlraytracing_amd.trueknn import TrueKNN, debug_box_tree  # noqa: F401

    lib = il.load()
    rng = np.random.default_rng(0)
    n, m, guard = 700, 300, 256
    P = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    S = torch.from_numpy((P[:m] + np.float32(0.002)).astype(np.float32)).cuda()
    N = torch.from_numpy(np.tile(np.float32([0, 0.6, 0.8]), (n, 1))).cuda()
    eng = TrueKNN(device=0)
    dev = eng.device
    bufs = {"d_corr": torch.full((m + guard,), -7, dtype=torch.int32, device=dev), "d_corr_dist": torch.full((m + guard,), -7.0, device=dev),
            "d_aligned": torch.full((3 * (m + guard),), -7.0, device=dev)}
    info = il.IcpInfo()
    init = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))

    def call(handle=None, options=True, with_info=True, init_values=None, outputs=tuple(bufs), **kw):
        o = il.IcpOptions()
        o.m, o.d_source, o.max_dist, o.max_iterations, o.rel_fitness, o.rel_rmse = m, S.data_ptr(), 0.05, 3, 1e-6, 1e-6
        for name in outputs:
            setattr(o, name, bufs[name].data_ptr())
        if init_values is not None:
            o.init = (ctypes.c_double * 16)(*init_values)
        for name, v in kw.items():
            setattr(o, name, v)
        info.correspondences, info.iterations, info.fitness, info.transform[5] = 99, 98, 97.0, 96.0
        rc = lib.tknnIcp(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info) if with_info else None, None)
        assert rc == 0 or (info.correspondences == 99 and info.iterations == 98 and info.fitness == 97.0 and info.transform[5] == 96.0), \
            "a refused call leaves the info alone"
        return rc

    def untouched(but=()):
        return all(bool((b == -7).all()) for name, b in bufs.items() if name not in but)

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnIcp: "), t
        return t

    plane = dict(method=il.METHODS["point_to_plane"], d_target_normals=N.data_ptr())
    # 1. missing pointers -- before the state
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(with_info=False) == ARG and "info" in text()
    assert call(d_source=None) == ARG and "d_source" in text()
    assert call(d_source=None, max_dist=-1.0) == ARG and "d_source" in text()
    # 2. not built, before any look at the values
    assert call() == STATE and "tknnBuild" in text()
    for bad in (dict(max_dist=0.0), dict(method=7), dict(robust=9), dict(flags=1), dict(max_iterations=-1), dict(m=-1), dict(rel_rmse=NAN)):
        assert call(**bad) == STATE
    assert call(d_source=None, m=0) == STATE, "m = 0 needs a tree too"
    # 3. a tree built with ids
    eng.build(P, ids=np.arange(n, dtype=np.int32)[::-1].copy())
    assert call() == UNSUPPORTED and "ids" in text()
    assert call(max_dist=-1.0, m=-1) == UNSUPPORTED
    assert call(d_source=None) == ARG and "d_source" in text()
    eng.build(P)
    # 4. the values, in the header's order
    for bad in (0.0, -1.0, NAN, INF, -INF):
        assert call(max_dist=bad) == ARG and "max_dist" in text()
    assert call(max_dist=0.0, method=5) == ARG and "max_dist" in text()
    for bad in (-1, 2, 100):
        assert call(method=bad) == ARG and "method" in text()
    assert call(method=2, robust=3) == ARG and "method" in text()
    for bad in (-1, 3, 50):
        assert call(robust=bad) == ARG and "robust" in text()
    assert call(robust=3, flags=1) == ARG and "robust" in text()
    for bad in (1, 2, 0x80000000):
        assert call(flags=bad) == ARG and "flag" in text()
    assert call(flags=1, method=il.METHODS["point_to_plane"]) == ARG and "flag" in text()
    assert call(method=il.METHODS["point_to_plane"]) == ARG and "d_target_normals" in text()
    assert call(method=il.METHODS["point_to_plane"], robust=1, robust_scale=0.0) == ARG and "d_target_normals" in text()
    for kind in (il.ROBUST["huber"], il.ROBUST["tukey"]):
        for bad in (0.0, -1.0, NAN, INF):
            assert call(robust=kind, robust_scale=bad) == ARG and "robust_scale" in text()
    assert call(robust=1, robust_scale=0.0, max_iterations=-1) == ARG and "robust_scale" in text()
    for bad in (-1, -100):
        assert call(max_iterations=bad) == ARG and "max_iterations" in text()
    assert call(max_iterations=-1, rel_fitness=-1.0) == ARG and "max_iterations" in text()
    for bad in (-1e-9, NAN, INF):
        assert call(rel_fitness=bad) == ARG and "rel_fitness" in text()
        assert call(rel_rmse=bad) == ARG and "rel_rmse" in text()
    assert call(rel_fitness=-1.0, rel_rmse=-1.0) == ARG and "rel_fitness" in text()
    for at in (0, 7, 15):
        for bad in (NAN, INF):
            values = np.eye(4).reshape(-1)
            values[at] = bad
            assert call(init_values=values) == ARG and "init" in text()
            assert call(init_values=values, m=-1) == ARG and "init" in text()
    assert call(m=-1) == ARG and " m " in text()
    assert call(m=2 ** 31 - 1) == ARG and " m " in text()
    assert untouched(), "a refused call writes nothing"
    # 5. no source points: success, T = init, everything else zero, nothing written
    values = np.eye(4).reshape(-1)
    values[3] = 0.25
    assert call(m=0, d_source=None, init_values=values) == 0 and list(info.transform) == list(values) and untouched()
    assert (info.correspondences, info.iterations, info.searches, info.fitness, info.inlier_rmse, info.solve_ms) == (0, 0, 0, 0, 0, 0)
    assert call(m=0) == 0 and list(info.transform) == list(np.eye(4).reshape(-1))
    # what the call does not read: robust_scale with L2
    assert call(robust_scale=NAN) == 0 and call(robust_scale=-1.0) == 0
    # the call itself; nothing is written behind the outputs, and an output that was not asked for stays untouched
    for b in bufs.values():
        b.fill_(-7)
    assert call(init=init) == 0 and info.iterations >= 1 and info.searches == info.iterations + 1 and info.correspondences == m and info.fitness == 1.0
    assert info.solve_ms >= info.search_ms > 0 and info.moment_ms > 0 and info.node_tests > 0 and info.point_tests > 0 and info.lane_rows == 0
    for name, b in bufs.items():
        width = 3 if name == "d_aligned" else 1
        assert (b[m * width:] == -7).all() and not (b[:m * width] == -7).any(), name
    everything = {name: b.clone() for name, b in bufs.items()}
    transform = list(info.transform)
    for name in bufs:
        for b in bufs.values():
            b.fill_(-7)
        assert call(outputs=(name,)) == 0 and untouched(but=(name,)) and list(info.transform) == transform
        assert torch.equal(bufs[name].view(torch.int32), everything[name].view(torch.int32)), name
    assert call(outputs=()) == 0 and list(info.transform) == transform
    assert call(outputs=(), **plane) == 0 and info.degenerate == 1 and info.iterations == 0, "every normal the same: no step"
    # a batched tree is a tree like any other: the labels are ignored
    eng.build(P, batch=(np.arange(n) % 3).astype(np.int32))
    assert call(outputs=()) == 0 and list(info.transform) == transform
    eng.close()


def test_the_wrapper_passes_the_codes_on():
    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    rng = np.random.default_rng(1)
    P = rng.uniform(0, 1, size=(200, 3)).astype(np.float32)
    eng = TrueKNN(device=0)
    with pytest.raises(TknnError) as err:
        eng.icp(P[:50], 0.1)
    assert err.value.code == STATE and str(err.value).count("tknnIcp") == 1
    eng.build(P, ids=np.arange(200, dtype=np.int32))
    with pytest.raises(TknnError) as err:
        eng.evaluate_registration(P[:50], 0.1)
    assert err.value.code == UNSUPPORTED and "ids" in str(err.value)
    eng.build(P)
    for bad in (0.0, -2.0, NAN):
        with pytest.raises(TknnError) as err:
            eng.icp(P[:50], bad)
        assert err.value.code == ARG and "max_dist" in str(err.value)
    with pytest.raises(TknnError) as err:
        eng.icp(P[:50], 0.1, max_iterations=-1)
    assert err.value.code == ARG and "max_iterations" in str(err.value)
    with pytest.raises(TknnError) as err:
        eng.icp(P[:50], 0.1, robust="tukey", robust_scale=0.0)
    assert err.value.code == ARG and "robust_scale" in str(err.value)
    bad = np.eye(4)
    bad[1, 3] = NAN
    with pytest.raises(TknnError) as err:
        eng.icp(P[:50], 0.1, init=bad)
    assert err.value.code == ARG and "init" in str(err.value)
    with pytest.raises(ValueError):
        eng.icp(P[:50], 0.1, method="point_to_plane", target_normals=np.zeros((199, 3), np.float32))
    r = eng.icp(np.zeros((0, 3), np.float32), 0.1, init=np.diag([1.0, 1.0, 1.0, 1.0]))
    assert r["iterations"] == 0 and r["fitness"] == 0 and np.array_equal(r["transform"].numpy(), np.eye(4))
    eng.close()


def test_a_box_tree_is_refused():
    """The engine's own tree is a point tree or none; a box tree lives behind the OWL groups.  What the call checks is that the
    engine's tree has points: an engine that never built one answers TKNN_E_STATE whatever else was built on the device."""
    import torch

    from owlraytracing_amd import _icp_lib as il
    from owlraytracing_amd.trueknn import TrueKNN, debug_box_tree

    boxes = np.float32([[0, 0, 0, 1, 1, 1], [2, 2, 2, 3, 3, 3], [4, 4, 4, 5, 5, 5], [1, 1, 1, 2, 2, 2]])
    assert len(debug_box_tree(boxes)["prim_id"]) == 4
    eng = TrueKNN(device=0)
    S = torch.zeros((4, 3), device=eng.device)
    o, info = il.IcpOptions(), il.IcpInfo()
    o.m, o.d_source, o.max_dist = 4, S.data_ptr(), 1.0
    info.iterations = 55
    assert il.load().tknnIcp(eng._h, ctypes.byref(o), ctypes.byref(info), None) == STATE and info.iterations == 55
    assert "no point tree" in il.load().tknnLastError().decode()
    eng.close()
