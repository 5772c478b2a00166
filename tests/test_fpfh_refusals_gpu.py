"""What tknnFpfh (include/owlknn_fpfh.h) refuses, one fault per row and in the header's order, that the message names the field, and
that a refused call writes nothing, neither outputs nor info; and what an accepted call leaves alone: the cells behind its n rows,
and every buffer it was not asked for."""
import ctypes

import numpy as np
import pytest

import fpfh_spec as fs

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3
OUTPUTS = {"d_fpfh": 33, "d_spfh": 33, "d_spfh_counts": 33, "d_counts": 1}


def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _fpfh_lib as fl
    from owlraytracing_amd.trueknn import TrueKNN

    lib = fl.load()
    c = fs.case("cube1025")
    n, guard, r = len(c["P"]), 1024, float(c["r"])
    eng = TrueKNN(device=0)
    dev = eng.device
    bufs = {name: torch.full(((n + guard) * width,), -7, dtype=torch.int32 if "counts" in name else torch.float32, device=dev) for name, width in OUTPUTS.items()}
    normals = torch.from_numpy(np.array(c["N"])).to(dev)
    info = fl.FpfhInfo()

    def call(handle=None, options=True, outputs=tuple(OUTPUTS), **kw):
        o = fl.FpfhOptions()
        o.radius, o.flags, o.d_normals = r, 0, normals.data_ptr()
        for name in outputs:
            setattr(o, name, bufs[name].data_ptr())
        for name, v in kw.items():
            setattr(o, name, v)
        info.total, info.node_tests, info.spfh_ms = 99, 98, 97.0
        rc = lib.tknnFpfh(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)
        assert rc == 0 or (info.total == 99 and info.node_tests == 98 and info.spfh_ms == 97.0), "a refused call leaves the info alone"
        return rc

    def untouched(but=()):
        return all(bool((b == -7).all()) for name, b in bufs.items() if name not in but)

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnFpfh: "), t
        return t

    # 1. missing pointers, no output -- before the state
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(outputs=()) == ARG and "no output" in text()
    assert call(outputs=(), d_normals=None) == ARG and "no output" in text()
    assert call(d_normals=None) == ARG and "d_normals" in text()
    assert call(d_normals=None, radius=-1.0) == ARG and "d_normals" in text()
    # 2. not built, before any look at the values
    assert call() == STATE and "tknnBuild" in text()
    for bad in (dict(radius=0.0), dict(radius=float("nan")), dict(flags=8)):
        assert call(**bad) == STATE
    eng.build(c["P"])
    assert call(outputs=(), radius=-1.0) == ARG and "no output" in text()
    assert call(d_normals=None, flags=8) == ARG and "d_normals" in text()
    # 3. the values, in the header's order
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(radius=bad) == ARG and "radius" in text()
        assert call(radius=bad, flags=8) == ARG and "radius" in text()
    for bad in (2, 8, 0x80000000, fl.FPFH_NO_SELF_TERM | 16):
        assert call(flags=bad) == ARG and "flag" in text()
    assert untouched(), "a refused call writes nothing"
    # the call itself; nothing is written behind the outputs
    hist, mem = c["hist"], c["mem"]
    assert call() == 0 and info.total == mem["lengths"].sum() and info.max_row == mem["lengths"].max() and info.skipped_pairs == hist["skipped"]
    assert info.fallback_items == 0 and info.node_tests > 0 and info.point_tests > 0
    assert info.solve_ms >= info.spfh_ms > 0 and info.fpfh_ms > 0 and info.stage_ms > 0
    assert np.array_equal(bufs["d_counts"][:n].cpu().numpy(), mem["lengths"])
    for name, width in OUTPUTS.items():
        assert (bufs[name][n * width:] == -7).all() and not (bufs[name][:n * width] == -7).any(), name
    everything = {name: b.clone() for name, b in bufs.items()}
    # every output asked alone: the same bits, and the buffers that were not asked for stay untouched
    for name in OUTPUTS:
        for b in bufs.values():
            b.fill_(-7)
        assert call(outputs=(name,)) == 0 and untouched(but=(name,))
        assert torch.equal(bufs[name].view(torch.int32), everything[name].view(torch.int32)), name
        assert (info.fpfh_ms > 0) == (name == "d_fpfh"), "the second pass runs for d_fpfh only"
    eng.close()


def test_the_wrapper_passes_the_codes_on():
    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    c = fs.case("n17")
    eng = TrueKNN(device=0)
    eng.n = len(c["P"])  # (the wrapper shapes the normals by it; the library has no tree yet)
    with pytest.raises(TknnError) as err:
        eng.fpfh(0.5, normals=c["N"])
    assert err.value.code == STATE and str(err.value).count("tknnFpfh") == 1
    eng.build(c["P"])
    for r in (0.0, -3.0, float("nan")):
        with pytest.raises(TknnError) as err:
            eng.fpfh(r, normals=c["N"])
        assert err.value.code == ARG and "radius" in str(err.value)
    eng.close()
