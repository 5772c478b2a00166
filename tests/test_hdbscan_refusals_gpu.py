"""What tknnLinkage, tknnHdbscanLabels and tknnHdbscan (include/owlknn_hdbscan.h) refuse, one fault per row and in the header's
order, and that a refused call writes nothing; then the argument checks of the wrappers above them."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import emst_spec as em  # noqa: E402
import hdbscan_spec as hs  # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = -1, -3, -5
MAX_K_REGISTERS = 64


class _Buffers:
    """Every output of the three calls, preset to -7, with room behind the rows the calls may write."""

    def __init__(self, torch, dev, n, guard=512):
        self.n = n
        mk = lambda rows, dtype: torch.full((rows + guard,), -7, dtype=dtype, device=dev)  # noqa: E731
        self.t = {"labels": mk(n, torch.int32), "parent": mk(2 * n - 1, torch.int32), "left": mk(n - 1, torch.int32), "right": mk(n - 1, torch.int32),
                  "size": mk(n - 1, torch.int32), "lambda": mk(n, torch.float64), "stability": mk(n - 1, torch.float64), "core_dist": mk(n, torch.float32),
                  "u": mk(n - 1, torch.int32), "v": mk(n - 1, torch.int32), "w": mk(n - 1, torch.float32)}

    def fill(self, o, names):
        for name in names:
            setattr(o, "d_" + name, self.t[name].data_ptr())

    def untouched(self, names=None):
        return all(bool((t == -7).all()) for name, t in self.t.items() if names is None or name in names)

    def reset(self):
        for t in self.t.values():
            t.fill_(-7)


def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _hdbscan_lib as hl
    from owlraytracing_amd.trueknn import TrueKNN

    lib = hl.load()
    P = hs.points("planar")[:500]
    n = len(P)
    tree = em.mst(P)
    want = hs.labels(n, tree["u"], tree["v"], tree["w"], 5)
    eng = TrueKNN(device=0)
    dev = eng.device
    b = _Buffers(torch, dev, n)
    u, v, w = (torch.from_numpy(np.array(tree[f])).to(dev) for f in ("u", "v", "w"))
    null = ctypes.c_void_p()

    def text(fn):
        t = lib.tknnLastError().decode()
        assert t.startswith(fn + ": "), t
        return t

    # ---- tknnLinkage: no tree is needed ----
    info = hl.LinkageInfo()
    info.rounds = 99

    def linkage(handle=None, options=True, **kw):
        o = hl.LinkageOptions()
        o.n, o.edges, o.d_u, o.d_v = n, n - 1, u.data_ptr(), v.data_ptr()
        b.fill(o, ("parent", "left", "right", "size"))
        for name, value in kw.items():
            setattr(o, name, value)
        return lib.tknnLinkage(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)

    assert linkage(handle=null) == ARG and "engine" in text("tknnLinkage")
    assert linkage(options=False) == ARG and "options" in text("tknnLinkage")
    assert linkage(d_u=None, n=0) == ARG and "d_u" in text("tknnLinkage")
    assert linkage(d_v=None, edges=n) == ARG and "d_v" in text("tknnLinkage")
    assert linkage(d_parent=None, d_left=None, d_right=None, d_size=None, n=0) == ARG and "d_parent" in text("tknnLinkage")
    for bad in ({"n": 0}, {"n": 1 << 30}, {"edges": -1}, {"edges": n}, {"n": n - 1}):
        assert linkage(**bad) == ARG and ("n" in text("tknnLinkage")), bad
    assert info.rounds == 99 and b.untouched(), "a refused call writes nothing"
    assert linkage() == 0 and info.roots == 1 and info.absorbed == n - 1 and info.host_edges == 0 and info.rounds >= 1 and info.solve_ms > 0
    for f in ("parent", "left", "right", "size"):
        rows = 2 * n - 1 if f == "parent" else n - 1
        assert np.array_equal(b.t[f][:rows].cpu().numpy(), want["dendrogram"][f]) and (b.t[f][rows:] == -7).all(), f
    # one output is enough; edges = 0 needs no records
    b.reset()
    assert linkage(d_parent=None, d_left=None, d_right=None) == 0 and b.untouched(("parent", "left", "right"))
    assert np.array_equal(b.t["size"][:n - 1].cpu().numpy(), want["dendrogram"]["size"])
    b.reset()
    assert linkage(edges=0, d_u=None, d_v=None) == 0 and info.roots == n and info.rounds == 0
    assert (b.t["parent"][:n] == -1).all() and (b.t["parent"][n:] == -7).all() and b.untouched(("left", "right", "size"))

    # ---- tknnHdbscanLabels ----
    b.reset()
    linfo = hl.HdbscanLabelsInfo()
    linfo.rounds = 99
    outputs = ("labels", "parent", "left", "right", "size", "lambda", "stability")

    def labels(handle=None, options=True, **kw):
        o = hl.HdbscanLabelsOptions()
        o.n, o.edges, o.d_u, o.d_v, o.d_w, o.min_cluster_size = n, n - 1, u.data_ptr(), v.data_ptr(), w.data_ptr(), 5
        b.fill(o, outputs)
        for name, value in kw.items():
            setattr(o, name, value)
        return lib.tknnHdbscanLabels(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(linfo), None)

    assert labels(handle=null) == ARG and "engine" in text("tknnHdbscanLabels")
    assert labels(options=False) == ARG and "options" in text("tknnHdbscanLabels")
    assert labels(d_labels=None, d_u=None) == ARG and "d_labels" in text("tknnHdbscanLabels")
    assert labels(d_u=None, d_w=None) == ARG and "d_u" in text("tknnHdbscanLabels")
    assert labels(d_v=None, n=0) == ARG and "d_v" in text("tknnHdbscanLabels")
    assert labels(d_w=None, min_cluster_size=1) == ARG and "d_w" in text("tknnHdbscanLabels")
    assert labels(n=0, min_cluster_size=1) == ARG and "n" in text("tknnHdbscanLabels")
    assert labels(edges=n, min_cluster_size=1) == ARG and "edges" in text("tknnHdbscanLabels")
    for mcs in (1, 0, -3):
        assert labels(min_cluster_size=mcs) == ARG and "min_cluster_size" in text("tknnHdbscanLabels")
    assert linfo.rounds == 99 and b.untouched(), "a refused call writes nothing"
    assert labels() == 0 and (linfo.clusters, linfo.noise, linfo.condensed_clusters) == (want["clusters"], want["noise"], want["condensed_clusters"])
    assert np.array_equal(b.t["labels"][:n].cpu().numpy(), want["labels"]) and (b.t["labels"][n:] == -7).all()
    assert np.array_equal(b.t["lambda"][:n].cpu().numpy(), want["lam"]) and (b.t["lambda"][n:] == -7).all() and (b.t["stability"][n - 1:] == -7).all()
    b.reset()
    assert labels(d_parent=None, d_left=None, d_right=None, d_size=None, d_lambda=None, d_stability=None) == 0
    assert np.array_equal(b.t["labels"][:n].cpu().numpy(), want["labels"]) and b.untouched(outputs[1:])

    # ---- tknnHdbscan ----
    b.reset()
    hinfo = hl.HdbscanInfo()
    hinfo.edges = 99
    everything = outputs + ("core_dist", "u", "v", "w")

    def hdbscan(handle=None, options=True, **kw):
        o = hl.HdbscanOptions()
        o.min_cluster_size, o.min_samples = 5, 3
        b.fill(o, everything)
        for name, value in kw.items():
            setattr(o, name, value)
        return lib.tknnHdbscan(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(hinfo), None)

    assert hdbscan(handle=null) == ARG and "engine" in text("tknnHdbscan")
    assert hdbscan(options=False) == ARG and "options" in text("tknnHdbscan")
    assert hdbscan(d_labels=None) == ARG and "d_labels" in text("tknnHdbscan")
    assert hdbscan() == STATE and "tknnBuild" in text("tknnHdbscan")
    assert hdbscan(min_cluster_size=1, min_samples=0) == STATE
    eng.build(P)
    assert hdbscan(d_labels=None, min_cluster_size=1) == ARG and "d_labels" in text("tknnHdbscan")
    assert hdbscan(min_cluster_size=1, min_samples=0) == ARG and "min_cluster_size" in text("tknnHdbscan")
    assert hdbscan(min_samples=0) == ARG and "min_samples" in text("tknnHdbscan")
    assert hdbscan(min_cluster_size=1, min_samples=MAX_K_REGISTERS + 2) == ARG
    assert hdbscan(min_samples=MAX_K_REGISTERS + 2) == UNSUPPORTED and "min_samples" in text("tknnHdbscan")
    assert hinfo.edges == 99 and b.untouched(), "a refused call writes nothing"
    assert hdbscan(min_samples=MAX_K_REGISTERS + 1, d_core_dist=None, d_u=None, d_v=None, d_w=None, d_parent=None, d_left=None, d_right=None, d_size=None,
                   d_lambda=None, d_stability=None) == 0, "the cap itself is served"
    assert hinfo.edges == n - 1 and hinfo.excluded == 0 and b.untouched(everything[1:])
    b.reset()
    ref = hs.labels(n, tree["u"], tree["v"], tree["w"], 5)
    assert hdbscan(min_samples=1) == 0 and np.array_equal(b.t["labels"][:n].cpu().numpy(), ref["labels"])
    assert b.untouched(("core_dist",)), "min_samples = 1 has no core distances"
    assert np.array_equal(b.t["u"][:n - 1].cpu().numpy(), tree["u"]) and all((b.t[f][n - 1:] == -7).all() for f in ("u", "v", "w", "left", "right", "size", "stability"))
    assert (b.t["parent"][2 * n - 1:] == -7).all() and (b.t["labels"][n:] == -7).all() and (b.t["lambda"][n:] == -7).all()
    assert hinfo.labels.solve_ms >= hinfo.emst_ms > 0 and hinfo.knn_ms == 0 and hinfo.labels.linkage_ms > 0
    eng.close()


def test_the_wrappers_check_their_arguments():
    import torch

    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    with pytest.raises(TknnError) as err:
        eng.hdbscan(5)
    assert err.value.code == STATE and str(err.value).count("tknnHdbscan") == 1
    u, v, w = np.int32([0, 1]), np.int32([1, 2]), np.float32([1, 2])
    for bad in ((u, v[:1], w), (u.astype(np.int64).tolist(), v, w), (torch.from_numpy(u), v, w), (u, v, None), (torch.from_numpy(u).cuda().long(), v, w)):
        with pytest.raises(ValueError):
            eng.hdbscan_labels(*bad, n=3, min_cluster_size=2)
    with pytest.raises(ValueError):
        eng.linkage(u, v, n=2)
    with pytest.raises(TknnError) as err:
        eng.hdbscan_labels(u, v, w, n=3, min_cluster_size=1)
    assert err.value.code == ARG
    got = eng.hdbscan_labels(u, v, w, n=3, min_cluster_size=2)
    assert got["labels"].cpu().tolist() == [-1, -1, -1] and set(got) == {"labels", "info"}, "one root cluster, which never wins"
    assert eng.linkage(u, v, n=4)["parent"].cpu().tolist() == [4, 4, 5, -1, 5, -1]
    eng.close()
