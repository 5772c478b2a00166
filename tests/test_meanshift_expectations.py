"""tests/meanshift_spec.py against itself, against sklearn and against the C ABI, without a GPU: the bound of one step admits an
honest fp32 evaluation in three orders of summation, also on a cloud at +1000, where the recipe that sums absolute coordinates does
not stay inside it; the float64 loop does on the blob set what the GPU tests ask of the device; the merge, the labels and bin_seeds
are sklearn's; include/owlknn_meanshift.h, owlraytracing_amd/_meanshift_lib.py and the built library agree."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  before the library is loaded (tests/test_cabi.py says why)

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import meanshift_spec as ms  # noqa: E402
import reduce_spec as rd  # noqa: E402

F = np.float32
SHIFT = F(1000.0)


def weight32(kernel, d2, r, h):
    """The weights as an fp32 evaluation of the header's formulas gives them, every operation rounded on its own."""
    d2 = d2.astype(F)
    if kernel == "flat":
        return np.ones_like(d2)
    k = rd.constants(kernel, r, h)
    if kernel == "gauss":
        return np.exp((d2 * k).astype(F)).astype(F)  # (numpy's float32 exp is within one ulp)
    return np.maximum(F(0), F(1) - d2 * k)


def pairwise32(t):
    t = t.astype(F)
    while len(t) > 1:
        if len(t) % 2:
            t = np.concatenate([t, np.zeros(1, F)])
        t = t[0::2] + t[1::2]
    return t[0] if len(t) else F(0)


def running32(t):
    return np.add.accumulate(t.astype(F), dtype=F)[-1] if len(t) else F(0)


ORDERS = (running32, lambda t: running32(t[::-1]), pairwise32)


def small_cloud(shift):
    """600 points and 80 seeds in a cube of edge 0.5 (about 12 neighbours within 0.08), moved by `shift` along every axis."""
    P = (np.random.default_rng(21).random((600, 3), dtype=F) * F(0.5) + F(shift)).astype(F)
    X = (np.random.default_rng(22).random((80, 3), dtype=F) * F(0.5) + F(shift)).astype(F)
    return P, X


def step32(P, X, r, kernel, h, order, absolute=False):
    """One step in fp32, the sums in `order`: (new (m,3) float32, wsum (m,) float32, shift (m,) float32).  absolute: the recipe that
    sums w p over the coordinates and divides, instead of w (p - x)."""
    mem = rd.members(P, X, r)
    new, wsum, shift = X.copy(), np.zeros(len(X), F), np.full(len(X), np.inf, F)
    for j in range(len(X)):
        lo, hi = mem["offsets"][j], mem["offsets"][j + 1]
        if hi == lo:
            continue
        w = weight32(kernel, mem["d2"][lo:hi], r, h)
        p = P[mem["idx"][lo:hi]]
        W = F(hi - lo) if kernel == "flat" else order(w)
        wsum[j] = W
        if absolute:
            new[j] = [order((w * p[:, c]).astype(F)) / W for c in range(3)]
            continue
        d = (p - X[j]).astype(F)
        s = np.array([order((w * d[:, c]).astype(F)) / W for c in range(3)], F)
        new[j] = X[j] + s
        shift[j] = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2], dtype=F)
    return new, wsum, shift


@pytest.mark.parametrize("kernel", ms.KERNELS)
@pytest.mark.parametrize("shift", (0.0, float(SHIFT)))
def test_the_bound_admits_an_honest_fp32_step_in_three_orders(kernel, shift):
    P, X = small_cloud(shift)
    r, h = F(0.08), F(0.03)
    if kernel == "gauss":
        r = F(0.09)
    want = ms.step(P, X, r, kernel, h)
    tol = ms.tolerances(want, kernel, r, h)
    has = want["len"] > 0
    assert has.mean() > 0.9 and 8 < want["len"].mean() < 30
    for order in ORDERS:
        new, wsum, sh = step32(P, X, r, kernel, h, order)
        assert (np.abs(new.astype(np.float64) - want["new"])[has] <= tol["new"][has]).all()
        assert (np.abs(wsum.astype(np.float64) - want["wsum"])[has] <= tol["wsum"][has]).all()
        assert (np.abs(sh.astype(np.float64) - want["shift"])[has] <= tol["shift"][has]).all()
        assert np.array_equal(new[~has], X[~has])


@pytest.mark.parametrize("kernel", ms.KERNELS)
def test_the_absolute_coordinate_recipe_leaves_the_bound_on_a_shifted_cloud(kernel):
    """sum w p / sum w in fp32 on the cloud at +1000: the sums carry sum|w p| ~ len * 1000 where the offsets carry len * r, so the
    mean is lost in the rounding of the coordinates.  Near the origin the same recipe is inside the bound up to x' being formed
    differently -- which is why the call sums offsets, and why the GPU tests hold it to this bound at +1000 too."""
    r, h = (F(0.09), F(0.03)) if kernel == "gauss" else (F(0.08), F(0.03))
    P, X = small_cloud(float(SHIFT))
    want = ms.step(P, X, r, kernel, h)
    tol = ms.tolerances(want, kernel, r, h)
    has = want["len"] > 1
    outside = []
    for order in ORDERS:
        new, _, _ = step32(P, X, r, kernel, h, order, absolute=True)
        over = (np.abs(new.astype(np.float64) - want["new"]) > tol["new"])[has]
        outside.append(over.any(axis=1).mean())
    print("rows of the absolute recipe outside the bound, per order:", outside)
    assert min(outside) > 0, "the recipe stays inside at this shift: raise the shift"


def test_the_step_by_hand():
    """Two points and a seed between them: flat -- the mean; count, W, the shift; distance exactly r is inside; nothing is self."""
    P = F([[0, 0, 0], [1, 0, 0]])
    st = ms.step(P, F([[0.25, 0, 0]]), 0.75, "flat")
    assert st["counts"][0] == 2 and st["wsum"][0] == 2 and np.allclose(st["new"][0], [0.5, 0, 0]) and np.isclose(st["shift"][0], 0.25)
    st = ms.step(P, F([[0.25, 0, 0]]), 0.5, "flat")
    assert st["counts"][0] == 1 and np.allclose(st["new"][0], [0, 0, 0])
    st = ms.step(P, F([[0, 0, 0], [5, 5, 5], [np.nan, 0, 0]]), 0.5, "gauss", 0.2)
    assert st["counts"].tolist() == [1, 0, 0] and st["shift"][0] == 0 and np.isnan(st["shift"][1])
    out = ms.loop(P, F([[0, 0, 0], [5, 5, 5], [np.nan, 0, 0], [0.25, 0, 0]]), 0.75, "flat", tol=1e-6, max_iterations=5)
    # row 0 is alone with the point it sits on: shift 0, converged after one step; row 3 moves to 0.5 and stays there
    assert out["status"].tolist() == [ms.CONVERGED, ms.EMPTY, ms.INVALID, ms.CONVERGED]
    assert out["iterations"].tolist() == [1, 0, 0, 2] and np.isinf(out["shift"][1:3]).all() and out["shift"][3] == 0
    assert np.array_equal(out["modes"][[0, 3]], F([[0, 0, 0], [0.5, 0, 0]])) and out["passes"] == 2 and out["walks"] == 5
    capped = ms.loop(P, F([[0.25, 0, 0]]), 0.75, "flat", tol=1e-6, max_iterations=1)
    assert capped["status"].tolist() == [ms.RUNNING] and capped["iterations"].tolist() == [1]


def test_the_float64_loop_on_the_blob_set_does_what_the_gpu_tests_ask():
    P, comp = ms.blobs()
    means = ms.blob_means()
    for kernel in ("flat", "gauss"):  # (measured: 4 and 8 passes, the farthest mode 0.0014 and 0.025 bandwidths from its mean)
        bw = ms.BLOB_KERNELS[kernel]["bandwidth"]
        out = ms.blob_loop(kernel)
        assert (out["status"] == ms.CONVERGED).all() and out["passes"] <= 10
        off = np.linalg.norm(out["modes"].astype(np.float64) - means[comp], axis=1).max()
        print(kernel, "passes", out["passes"], "walks", out["walks"], "farthest mode / bandwidth", off / bw)
        assert off <= 0.05 * bw
        assert out["walks"] < len(P) * out["passes"], "seeds stop at different passes: the active set shrinks"
        res = ms.merge_and_label(P, out["modes"], out["counts"] if kernel == "flat" else out["wsum"], out["status"], out["counts"], bw)
        assert len(res["centers"]) == 4 and ms.same_partition(res["labels"], comp)
        assert np.all(np.diff(res["scores"]) <= 0)
        far = np.linalg.norm(res["centers"].astype(np.float64)[:, None] - means[None], axis=2).min(axis=1)
        assert (far <= 0.05 * bw).all()


def test_merge_labels_and_bin_seeds_are_sklearns():
    cluster = pytest.importorskip("sklearn.cluster")
    P, comp = ms.blobs()
    bw = ms.BLOB_KERNELS["flat"]["bandwidth"]
    sk = cluster.MeanShift(bandwidth=bw, cluster_all=True).fit(P)
    out = ms.blob_loop("flat")
    res = ms.merge_and_label(P, out["modes"], out["counts"], out["status"], out["counts"], bw)
    assert len(res["centers"]) == len(sk.cluster_centers_) == 4
    d = np.linalg.norm(res["centers"].astype(np.float64)[:, None] - sk.cluster_centers_[None], axis=2)
    assert (d.min(axis=1) <= 1e-3 * bw).all() and sorted(d.argmin(axis=1).tolist()) == [0, 1, 2, 3], "the same set of centres"
    assert ms.same_partition(res["labels"], sk.labels_)
    # two outliers: sklearn makes each a cluster of its own, and so does min_count = 1; cluster_all False orphans nobody then
    Q = np.concatenate([P, F([[0.5, 0.5, 0.05], [0.05, 0.95, 0.05]])])
    sk = cluster.MeanShift(bandwidth=bw, cluster_all=False).fit(Q)
    out = ms.loop(Q, None, F(bw), "flat", tol=1e-3 * bw, max_iterations=300)
    res = ms.merge_and_label(Q, out["modes"], out["counts"], out["status"], out["counts"], bw, cluster_all=False)
    assert len(res["centers"]) == len(sk.cluster_centers_) == 6
    both = (res["labels"] >= 0) & (sk.labels_ >= 0)  # (sklearn measures its orphans from its own centres, a rounding away)
    assert both.mean() > 0.999 and ms.same_partition(res["labels"][both], sk.labels_[both])
    # min_count = 2 takes the lone seeds out of the candidates: the outliers are orphans
    res = ms.merge_and_label(Q, out["modes"], out["counts"], out["status"], out["counts"], bw, cluster_all=False, min_count=2)
    assert len(res["centers"]) == 4 and (res["labels"][-2:] == -1).all() and ms.same_partition(res["labels"][:-2][res["labels"][:-2] >= 0], comp[res["labels"][:-2] >= 0])
    for pts, size, freq in ((P, bw, 1), (P, bw, 5), ((P - F(0.5)) * F(3), 0.25, 2)):
        mine = ms.bin_seeds(pts, size, freq)
        theirs = np.asarray(cluster.get_bin_seeds(np.asarray(pts), size, freq), np.float32)
        assert len(mine) > 4 and {tuple(x) for x in np.round(mine / F(size)).astype(int).tolist()} == {tuple(x) for x in np.round(theirs / F(size)).astype(int).tolist()}
        assert np.allclose(np.sort(mine, axis=0), np.sort(theirs, axis=0), atol=1e-6)
        again = ms.bin_seeds(pts[::-1], size, freq)
        assert np.array_equal(mine, again), "the seeds do not depend on the order of the points"


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"TKNN_API[^;(]*?\b(tknn\w+)\s*\(", text))


def test_header_binding_and_struct_layouts_agree(tmp_path):
    """tknnMeanShift is declared in its own header, exported and bound with its signature, nothing was added to owlknn.h or to _lib's
    tables, and the ctypes records have the header's sizes and offsets (gcc, C99)."""
    from owlraytracing_amd import _lib, _meanshift_lib, _reduce_lib

    assert _declared("owlknn_meanshift.h") == set(_meanshift_lib.SIGNATURES) == {"tknnMeanShift"}
    assert "tknnMeanShift" not in _declared("owlknn.h") and "tknnMeanShift" not in _lib.SIGNATURES and "tknnMeanShift" not in _reduce_lib.SIGNATURES
    res, args = _meanshift_lib.SIGNATURES["tknnMeanShift"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.POINTER(_meanshift_lib.MeanShiftOptions), ctypes.POINTER(_meanshift_lib.MeanShiftInfo), ctypes.c_void_p]
    pairs = {"tknnMeanShiftOptions": _meanshift_lib.MeanShiftOptions, "tknnMeanShiftInfo": _meanshift_lib.MeanShiftInfo}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn_meanshift.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    consts = {"TKNN_MS_RUNNING": _meanshift_lib.MS_RUNNING, "TKNN_MS_CONVERGED": _meanshift_lib.MS_CONVERGED, "TKNN_MS_EMPTY": _meanshift_lib.MS_EMPTY,
              "TKNN_MS_INVALID": _meanshift_lib.MS_INVALID, "TKNN_W_ONE": _meanshift_lib.KERNELS["flat"], "TKNN_W_GAUSS": _meanshift_lib.KERNELS["gauss"],
              "TKNN_W_EPANECHNIKOV": _meanshift_lib.KERNELS["epanechnikov"]}
    for cname in consts:
        lines.append('  printf("const %s %%ld\\n", (long)%s);' % (cname, cname))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        cname, what, value = line.split()
        if cname == "const":
            assert consts[what] == int(value), what
        elif what == "size":
            assert ctypes.sizeof(pairs[cname]) == int(value), cname
        else:
            assert getattr(pairs[cname], what).offset == int(value), (cname, what)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in pairs.values()) + len(consts)
    assert (ms.RUNNING, ms.CONVERGED, ms.EMPTY, ms.INVALID) == (_meanshift_lib.MS_RUNNING, _meanshift_lib.MS_CONVERGED, _meanshift_lib.MS_EMPTY, _meanshift_lib.MS_INVALID)
    lib = _meanshift_lib.load()
    assert lib is _lib.load() and lib.tknnMeanShift.restype is ctypes.c_int and lib.tknnMeanShift.argtypes == args
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT tknnMeanShift$", exported, flags=re.M), "the library exports the symbol"


def test_a_null_engine_is_refused_without_a_device():
    from owlraytracing_amd import _meanshift_lib

    lib = _meanshift_lib.load()
    o, info = _meanshift_lib.MeanShiftOptions(), _meanshift_lib.MeanShiftInfo()
    info.walks = 77
    assert lib.tknnMeanShift(None, ctypes.byref(o), ctypes.byref(info), None) == -1
    assert lib.tknnLastError().decode().startswith("tknnMeanShift: ") and "engine" in lib.tknnLastError().decode() and info.walks == 77


def test_the_package_exports_the_calls():
    import owlraytracing_amd
    from owlraytracing_amd import trueknn

    assert callable(owlraytracing_amd.mean_shift) and callable(owlraytracing_amd.bin_seeds)
    assert callable(trueknn.mean_shift) and callable(trueknn.bin_seeds)
    assert callable(trueknn.TrueKNN.mean_shift) and callable(trueknn.TrueKNN.mean_shift_modes)
