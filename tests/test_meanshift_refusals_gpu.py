"""What tknnMeanShift (include/owlknn_meanshift.h) refuses, one fault per row and in the header's order, that the message names the
field, and that a refused call writes nothing, neither outputs nor info; the raw call with each output alone; the trees it takes."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3
NAN, INF = float("nan"), float("inf")
WIDTH = {"d_modes": 3}


def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _meanshift_lib as ml
    from owlraytracing_amd.trueknn import TrueKNN

    lib = ml.load()
    rng = np.random.default_rng(0)
    n, m, guard = 700, 300, 256
    P = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    S = torch.from_numpy(rng.uniform(0, 1, size=(m, 3)).astype(np.float32)).cuda()
    eng = TrueKNN(device=0)
    dev = eng.device
    rows = max(n, m) + guard
    bufs = {"d_modes": torch.full((3 * rows,), -7.0, device=dev), "d_counts": torch.full((rows,), -7, dtype=torch.int32, device=dev),
            "d_wsum": torch.full((rows,), -7.0, device=dev), "d_shift": torch.full((rows,), -7.0, device=dev),
            "d_iterations": torch.full((rows,), -7, dtype=torch.int32, device=dev), "d_status": torch.full((rows,), 249, dtype=torch.uint8, device=dev)}
    blank = {name: b.clone() for name, b in bufs.items()}
    info = ml.MeanShiftInfo()

    def call(handle=None, options=True, with_info=True, outputs=tuple(bufs), **kw):
        o = ml.MeanShiftOptions()
        o.m, o.d_seeds, o.radius, o.bandwidth, o.tol, o.weight, o.max_iterations = m, S.data_ptr(), 0.15, 0.05, 1e-4, ml.KERNELS["flat"], 8
        for name in outputs:
            setattr(o, name, bufs[name].data_ptr())
        for name, v in kw.items():
            setattr(o, name, v)
        info.walks, info.iterations, info.converged, info.solve_ms = 99, 98, 97, 96.0
        rc = lib.tknnMeanShift(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info) if with_info else None, None)
        assert rc == 0 or (info.walks == 99 and info.iterations == 98 and info.converged == 97 and info.solve_ms == 96.0), "a refused call leaves the info alone"
        return rc

    def untouched(but=()):
        return all(torch.equal(b, blank[name]) for name, b in bufs.items() if name not in but)

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnMeanShift: "), t
        return t

    gauss = ml.KERNELS["gauss"]
    # 1. missing pointers, no output, own points with m != n -- before the state
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(with_info=False) == ARG and "info" in text()
    assert call(outputs=()) == ARG and "no output" in text()
    assert call(outputs=(), radius=-1.0) == ARG and "no output" in text()
    assert call(d_seeds=None) == ARG and "m must equal n" in text()
    # 2. not built, before any look at the values
    assert call() == STATE and "tknnBuild" in text()
    for bad in (dict(radius=0.0), dict(weight=7), dict(flags=1), dict(max_iterations=0), dict(m=-1), dict(tol=NAN)):
        assert call(**bad) == STATE
    assert call(m=0) == STATE, "m = 0 needs a tree too"
    eng.build(P)
    assert call(d_seeds=None) == ARG and "m must equal n" in text()
    assert call(d_seeds=None, m=n + 1, radius=-1.0) == ARG and "m must equal n" in text()
    # 3. the values, in the header's order
    for bad in (0.0, -1.0, NAN, INF, -INF):
        assert call(radius=bad) == ARG and "radius" in text()
    assert call(radius=0.0, weight=5) == ARG and "radius" in text()
    for bad in (-1, 3, 4, 100):  # 3: TKNN_W_CUBIC_SPLINE is no mean-shift kernel
        assert call(weight=bad) == ARG and "weight" in text()
    assert call(weight=3, bandwidth=-1.0, tol=-1.0) == ARG and "weight" in text()
    for bad in (0.0, -1.0, NAN, INF):
        assert call(weight=gauss, bandwidth=bad) == ARG and "bandwidth" in text()
    assert call(weight=gauss, bandwidth=0.0, tol=-1.0) == ARG and "bandwidth" in text()
    for bad in (-1e-9, -1.0, NAN, INF):
        assert call(tol=bad) == ARG and "tol" in text()
    assert call(tol=-1.0, max_iterations=0) == ARG and "tol" in text()
    for bad in (0, -1, -100):
        assert call(max_iterations=bad) == ARG and "max_iterations" in text()
    assert call(max_iterations=0, flags=1) == ARG and "max_iterations" in text()
    for bad in (1, 2, 0x80000000):
        assert call(flags=bad) == ARG and "flag" in text()
    assert call(flags=1, m=-1) == ARG and "flag" in text()
    assert call(m=-1) == ARG and " m " in text()
    assert call(m=2 ** 31 - 1) == ARG and " m " in text()
    assert untouched(), "a refused call writes nothing"
    # 4. no seeds: success, a zeroed info, nothing written
    assert call(m=0) == 0 and untouched()
    assert (info.iterations, info.walks, info.converged, info.empty, info.running, info.invalid, info.solve_ms, info.walk_ms) == (0,) * 8
    # what the call does not read: the bandwidth without TKNN_W_GAUSS
    assert call(bandwidth=NAN) == 0 and call(bandwidth=-1.0, weight=ml.KERNELS["epanechnikov"]) == 0
    # the call itself; nothing is written behind the outputs, and an output that was not asked for stays untouched
    for name, b in bufs.items():
        b.copy_(blank[name])
    assert call() == 0 and 1 <= info.iterations <= 8 and m <= info.walks <= 8 * m
    assert info.converged + info.empty + info.running + info.invalid == m and info.converged > 0
    assert info.solve_ms >= info.walk_ms > 0 and info.order_ms > 0 and info.node_tests > 0 and info.point_tests > 0 and info.fallback_items == 0
    for name, b in bufs.items():
        w = WIDTH.get(name, 1)
        assert torch.equal(b[m * w:], blank[name][m * w:]) and not (b[:m * w] == blank[name][:m * w]).any(), name
    everything = {name: b.clone() for name, b in bufs.items()}
    walks = info.walks
    for name in bufs:
        for other, b in bufs.items():
            b.copy_(blank[other])
        assert call(outputs=(name,)) == 0 and untouched(but=(name,)) and info.walks == walks
        assert torch.equal(bufs[name], everything[name]), name
    # the own points: by row, m = n
    for name, b in bufs.items():
        b.copy_(blank[name])
    assert call(d_seeds=None, m=n) == 0 and info.walks >= n
    for name, b in bufs.items():
        w = WIDTH.get(name, 1)
        assert torch.equal(b[n * w:], blank[name][n * w:]) and not (b[:n * w] == blank[name][:n * w]).any(), name
    own = {name: b.clone() for name, b in bufs.items()}
    # a tree with ids and a batched tree are trees like any other
    eng.build(P, ids=np.arange(n, dtype=np.int32)[::-1].copy())
    assert call(d_seeds=None, m=n) == 0 and all(torch.equal(bufs[name], own[name]) for name in bufs)
    eng.build(P, batch=(np.arange(n) % 3).astype(np.int32))
    assert call(outputs=("d_counts",), max_iterations=1) == 0
    assert torch.equal(bufs["d_counts"][:m], eng.radius_reduce(0.15, queries=S, want_wsum=False)["counts"]), "the labels are ignored"
    eng.close()


def test_the_wrapper_passes_the_codes_on():
    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    rng = np.random.default_rng(1)
    P = rng.uniform(0, 1, size=(200, 3)).astype(np.float32)
    eng = TrueKNN(device=0)
    with pytest.raises(TknnError) as err:
        eng.mean_shift_modes(0.1, seeds=P[:50])
    assert err.value.code == STATE and str(err.value).count("tknnMeanShift") == 1
    eng.build(P)
    for bad in (0.0, -2.0, NAN):
        with pytest.raises(TknnError) as err:
            eng.mean_shift_modes(0.1, seeds=P[:50], radius=bad)
        assert err.value.code == ARG and "radius" in str(err.value)
    with pytest.raises(TknnError) as err:
        eng.mean_shift_modes(-0.1, seeds=P[:50], kernel="gauss", radius=0.3, tol=0.0)
    assert err.value.code == ARG and "bandwidth" in str(err.value)
    with pytest.raises(TknnError) as err:
        eng.mean_shift_modes(0.1, seeds=P[:50], max_iterations=0)
    assert err.value.code == ARG and "max_iterations" in str(err.value)
    with pytest.raises(TknnError) as err:
        eng.mean_shift_modes(0.1, seeds=P[:50], tol=-1.0)
    assert err.value.code == ARG and "tol" in str(err.value)
    with pytest.raises(ValueError):
        eng.mean_shift_modes(0.1, kernel="cubic_spline")
    r = eng.mean_shift_modes(0.1, seeds=np.zeros((0, 3), np.float32))
    assert tuple(r["modes"].shape) == (0, 3) and r["info"]["walks"] == 0 and r["info"]["iterations"] == 0
    eng.close()


def test_an_engine_without_a_point_tree_is_refused():
    """The engine's own tree is a point tree or none; a box tree lives behind the OWL groups.  What the call checks is that the
    engine's tree has points: an engine that never built one answers TKNN_E_STATE whatever else was built on the device."""
    import torch

    from owlraytracing_amd import _meanshift_lib as ml
    from owlraytracing_amd.trueknn import TrueKNN, debug_box_tree

    boxes = np.float32([[0, 0, 0, 1, 1, 1], [2, 2, 2, 3, 3, 3], [4, 4, 4, 5, 5, 5], [1, 1, 1, 2, 2, 2]])
    assert len(debug_box_tree(boxes)["prim_id"]) == 4
    eng = TrueKNN(device=0)
    S = torch.zeros((4, 3), device=eng.device)
    out = torch.zeros((4, 3), device=eng.device)
    o, info = ml.MeanShiftOptions(), ml.MeanShiftInfo()
    o.m, o.d_seeds, o.radius, o.max_iterations, o.d_modes = 4, S.data_ptr(), 1.0, 1, out.data_ptr()
    info.iterations = 55
    assert ml.load().tknnMeanShift(eng._h, ctypes.byref(o), ctypes.byref(info), None) == STATE and info.iterations == 55
    assert "no point tree" in ml.load().tknnLastError().decode()
    eng.close()
