"""The spec of tknnSegmentPlane (tests/plane_spec.py) against hand-worked cases, without a GPU: three points and their plane, a
collinear sample, a point at exactly the threshold, the angle rule, the sign rule, the refit kept and rejected; the sample of a trial
is tknnRansac's; the eigen-solver of owlraytracing_amd/csrc/plane_solve.h, compiled for the host, gives the spec's fp32 normal bit
for bit; the ctypes records of owlraytracing_amd/_plane_lib.py have the header's layout and the library exports the symbol."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_spec as ps  # noqa: E402
import ransac_sample_host  # noqa: E402

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def plane_of(p0, p1, p2, **kw):
    """The spec's trial on a cloud of exactly these three rows, whichever order the sample draws them in: (status, normal, anchor)."""
    P = np.array([p0, p1, p2], F)
    for t in range(64):
        st, nm, an, idx = ps.trial_planes(P, np.arange(3), 0, [t], **kw)
        if st[0] != ps.DUPLICATE and idx[0].tolist() == [0, 1, 2]:
            return st[0], nm[0], an[0]
    raise AssertionError("no trial of 64 draws the rows in order")


def test_three_points_and_their_plane():
    st, n, a = plane_of((1, 2, 3), (3, 2, 3), (1, 5, 3))
    assert st == ps.OK and n.tolist() == [0.0, 0.0, 1.0] and a.tolist() == [1.0, 2.0, 3.0]  # e1 = (2,0,0), e2 = (0,3,0), g = (0,0,6)
    st, n, a = plane_of((0, 0, 0), (1, 0, 1), (0, 1, 0))  # g = (0*0 - 1*1, 1*0 - 1*0, 1*1 - 0*0) = (-1, 0, 1)
    r = F(1) / np.sqrt(F(2))
    assert st == ps.OK and np.array_equal(bits(n), bits([-r, F(0), r]))
    plane, sign = ps.output_plane(n, a)
    assert sign == -1.0 and plane.tolist() == [float(r), 0.0, -float(r), 0.0], "the first nonzero entry is made positive"
    plane, sign = ps.output_plane(n, a, axis=(0, 0, 5))
    assert sign == 1.0 and plane[2] > 0, "with an axis the normal is turned towards it"
    plane, sign = ps.output_plane(n, a, axis=(0, 3, 0))
    assert sign == -1.0, "a zero dot with the axis falls back to the first nonzero entry"


def test_a_collinear_sample_is_degenerate():
    assert plane_of((0, 0, 0), (1, 1, 1), (2, 2, 2))[0] == ps.DEGENERATE
    assert plane_of((0, 0, 0), (0, 0, 0), (1, 2, 3))[0] == ps.DEGENERATE, "a repeated point: g2 = 0 is not > 0"
    assert plane_of((0, 0, 0), (1, 0, 0), (0, 2.0 ** -19, 0))[0] == ps.OK, "g2 = 2^-38 > 2^-40 * (1 * 2^-38)"
    assert plane_of((0, 0, 0), (1, 0, 0), (1, 2.0 ** -21, 0))[0] == ps.DEGENERATE, "g2 = 2^-42 is not > 2^-40 * (1 * (1 + 2^-42))"
    assert plane_of((0, 0, 0), (3e19, 0, 0), (0, 3e19, 0))[0] == ps.DEGENERATE, "g2 overflows: not finite"


def test_a_point_at_exactly_the_threshold_is_an_inlier():
    n, a = F([0, 0, 1]), F([0.25, 0.5, 0.125])
    X = F([[7, -3, 0.25], [7, -3, 0.0], [0, 0, 0.2500001], [0, 0, np.nan], [np.inf, 0, 0.125]])
    d = ps.distances(n, a, X)[0]
    assert d[:2].tolist() == [0.125, 0.125] and (d[:2] <= F(0.125)).all() and not d[2] <= F(0.125)
    assert np.isnan(d[3]) and np.isnan(d[4]), "0 * inf: a row that is not finite is no inlier, whatever the plane"
    ev = ps.evaluate(X, ps.active_rows(X), n, a, 0.125)
    assert ev["rows"].tolist() == [0, 1] and ev["mask"].tolist() == [1, 1, 0, 0, 0] and ev["rmse"] == 0.125


def test_the_angle_rule():
    tilted = ((0, 0, 0), (1, 0, 0.125), (0, 1, 0))  # g = (-0.125, 0, 1): |cos| with z = 1 / sqrt(1.015625) = 0.99227...
    assert plane_of(*tilted, axis=(0, 0, 1), min_cos=0.99)[0] == ps.OK
    assert plane_of(*tilted, axis=(0, 0, -4), min_cos=0.99)[0] == ps.OK, "the absolute value: the axis' sign and length do not matter"
    assert plane_of(*tilted, axis=(0, 0, 1), min_cos=0.995)[0] == ps.ANGLE
    assert plane_of(*tilted, axis=(1, 0, 0), min_cos=0.99)[0] == ps.ANGLE
    assert plane_of(*tilted, axis=(0, 0, 0), min_cos=0.99)[0] == ps.OK, "an all-zero axis is no constraint"
    assert plane_of((0, 0, 0), (1, 0, 0), (0, 1, 0), axis=(0, 0, 1), min_cos=1.0)[0] == ps.OK, "|cos| = 1 >= 1"


def test_the_refit_keeps_or_rejects():
    rng = np.random.default_rng(3)
    uv = rng.random((400, 2))
    P = np.concatenate([np.stack([uv[:, 0], uv[:, 1], 0.5 + 0.001 * rng.standard_normal(400)], axis=1), rng.random((100, 3))]).astype(F)
    A, thr = ps.active_rows(P), 0.01
    start = ps.evaluate(P, A, F([0.02, 0.0, 1.0]) / np.sqrt(F(1.0004)), F([0.5, 0.5, 0.5]), thr)  # a tilted start
    fit = ps.refit(P, start["rows"], ps.scene_centre(P))
    after = ps.evaluate(P, A, fit["normal"], fit["anchor"], thr)
    assert after["inliers"] >= start["inliers"] and abs(abs(fit["normal"][2]) - 1) < 1e-4 and fit["tol_normal"] < 2e-7, "kept: not fewer inliers"
    # rejected: the inliers of a slab through uniform clutter are spread evenly over the slab: the smallest axis of their covariance
    # is the slab's own, the refit turns the plane by next to nothing, and the count it finds can be smaller
    lam, v = ps.jacobi(np.diag([3.0, 1.0, 2.0]))
    assert lam == [3.0, 1.0, 2.0] and v == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], "a diagonal matrix is left alone"
    line = np.stack([np.arange(10), np.zeros(10), np.zeros(10)], axis=1).astype(F)
    assert ps.refit(line, np.arange(10), np.zeros(3)) is None, "points on a line: the two smallest eigenvalues are equal, the refit stops"
    assert ps.refit(P, np.arange(0), np.zeros(3)) is None
    M = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.25], [0.5, 0.25, 1.0]])
    lam, v = ps.jacobi(M)
    w, _ = np.linalg.eigh(M)
    assert np.allclose(sorted(lam), w, rtol=1e-14) and np.allclose(np.array(v) @ np.diag(lam) @ np.array(v).T, M, atol=1e-14)


def test_the_sample_is_ransacs():
    for seed, c in ((7, 3), (7, 4), (0, 1025), (12345, 65553), (2 ** 32 - 1, 2 ** 31 - 2)):
        t = np.arange(0, 3000, 7)
        idx, ok = ps.global_spec.samples(seed, t, 3, c)
        hidx, hok = ransac_sample_host.samples(np.full(len(t), seed, np.uint32), t, np.full(len(t), 3), np.full(len(t), c, np.uint32))
        assert np.array_equal(ok, hok) and np.array_equal(idx[ok], hidx[ok][:, :3])
    c, want = ps.case("n3")
    st, _, _, idx = ps.trial_planes(c["P"], want["A"], c["seed"], np.arange(c["trials"]))
    hidx, hok = ransac_sample_host.samples(np.full(c["trials"], c["seed"], np.uint32), np.arange(c["trials"]), np.full(c["trials"], 3), np.full(c["trials"], 3, np.uint32))
    assert np.array_equal(st == ps.DUPLICATE, ~hok) and np.array_equal(idx[hok], hidx[hok][:, :3])


def test_the_cases_are_what_they_say():
    assert ps.case("n2")[1]["trials_run"] == 0 and ps.case("n2")[1]["best_trial"] == -1
    for name in ps.CASES:
        c, want = ps.case(name)
        if want["active"] >= 3:
            assert want["trials_run"] == c["trials"] == ps.BATCH + 7 and want["batches"] == 2, name
    assert ps.case("n3")[1]["status_counts"][ps.DUPLICATE] > 0
    assert ps.case("duplicates")[1]["status_counts"][ps.DEGENERATE] > 0
    both = ps.case("duplicates_c4")[1]
    assert both["active"] == 4 and both["status_counts"][ps.DUPLICATE] > 0 and both["status_counts"][ps.DEGENERATE] > 0
    assert 0 < ps.case("axis")[1]["status_counts"][ps.ANGLE] < ps.TRIALS and ps.case("axis")[1]["status_counts"][ps.OK] > 0
    c, want = ps.case("nan_inf")
    assert want["active"] == len(c["P"]) - 60 and np.isnan(c["P"]).any() and np.isinf(c["P"]).any()
    c, want = ps.case("active_half")
    order = ps.sorted_order(c["P"])
    per_block = c["active"][order[:64 * 16]].reshape(-1, 16).sum(axis=1)
    assert (per_block[[1, 2, 5]] == 0).all() and per_block[3] == 1 and abs(want["active"] / len(c["P"]) - 0.5) < 0.05
    c, want = ps.case("wide")
    assert (want["inliers"][want["status"] == ps.OK] == want["active"]).all()
    c, want = ps.case("lattice")
    st, nm, an, _ = ps.trial_planes(c["P"], want["A"], c["seed"], np.arange(c["trials"]))
    flat = (st == ps.OK) & ((np.abs(nm) == 1).sum(axis=1) == 1)
    d = ps.distances(nm[flat], an[flat], c["P"])
    assert flat.sum() >= 5 and (d == F(c["thr"])).any(axis=1).all(), "axis-aligned trials with points at exactly the threshold"
    assert np.array_equal(ps.case("shifted")[1]["status"], ps.case("plane_clutter")[1]["status"])
    assert ps.case("cube65553")[0]["P"].shape == (16 * 64 * 64 + 17, 3)


def test_the_stop_rule():
    c, _ = ps.case("plane_clutter")
    early = ps.segment(c["P"], c["thr"], 8 * ps.BATCH, c["seed"], confidence=0.999)
    assert early["trials_run"] == ps.BATCH and early["batches"] == 1 and (early["status"][ps.BATCH:] == -1).all(), "f about 0.5: 52 trials are enough"
    never = ps.segment(c["P"], c["thr"], 2 * ps.BATCH, c["seed"], confidence=1.0)
    assert never["trials_run"] == 2 * ps.BATCH and np.array_equal(never["status"][:ps.BATCH], early["status"][:ps.BATCH]), "a trial does not depend on its batch"


SOLVE_SHIM = r"""
#include "plane_solve.h"
extern "C" int refit(const double *mom, const double *centre, float *normal, float *anchor) { return owlmi::plane_refit(mom, centre, normal, anchor) ? 1 : 0; }
extern "C" double output(const float *normal, const float *anchor, int has_axis, const float *axis, double *plane) {
  float unit[3];
  const bool has = has_axis && owlmi::plane_axis(axis, unit);
  return owlmi::plane_output(normal, anchor, has, unit, plane);
}
"""


def test_the_host_solver_gives_the_specs_plane_bit_for_bit(tmp_path):
    """plane_solve.h compiled with the host compiler, fed the spec's own moments: the same operations in the same order, so the fp32
    normal and anchor, and the output plane, are equal bit for bit (the device's moments differ in their last bits: the header's
    tolerance is for those)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    src, so = tmp_path / "shim.cpp", tmp_path / "libplanesolve.so"
    src.write_text(SOLVE_SHIM)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "owlraytracing_amd", "csrc"), str(src), "-o", str(so)],
                   check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(str(so))
    lib.output.restype = ctypes.c_double
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for name in ("plane_clutter", "shifted", "n1025", "lattice"):
        c, want = ps.case(name)
        rows = ps.evaluate(c["P"], want["A"], want["normal"], want["anchor"], c["thr"])["rows"]
        centre = ps.scene_centre(c["P"])
        X = c["P"][rows].astype(np.float64) - centre
        S2 = X.T @ X
        mom = np.array([len(X), 0.0, *X.sum(axis=0), S2[0, 0], S2[0, 1], S2[0, 2], S2[1, 1], S2[1, 2], S2[2, 2]])
        normal, anchor = np.zeros(3, F), np.zeros(3, F)
        fit = ps.refit(c["P"], rows, centre)
        assert lib.refit(ptr(mom), ptr(centre), ptr(normal), ptr(anchor)) == (fit is not None) == 1, name
        assert np.array_equal(bits(normal), bits(fit["normal"])) and np.array_equal(bits(anchor), bits(fit["anchor"])), name
        for axis in (None, (0.0, 0.0, -2.0)):
            plane = np.zeros(4)
            sign = lib.output(ptr(normal), ptr(anchor), int(axis is not None), ptr(np.array(axis or (0, 0, 0), F)), ptr(plane))
            wplane, wsign = ps.output_plane(normal, anchor, axis)
            assert sign == wsign and np.array_equal(plane.view(np.uint64), wplane.view(np.uint64)), (name, axis)
    line = np.array([10.0, 0.0, 45.0, 0.0, 0.0, 285.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    assert lib.refit(ptr(line), ptr(np.zeros(3)), ptr(normal), ptr(anchor)) == 0, "points on a line: the refit stops"


def test_records_have_the_headers_sizes(tmp_path):
    from owlraytracing_amd import _lib, _plane_lib

    pairs = {"tknnPlaneOptions": _plane_lib.PlaneOptions, "tknnPlaneInfo": _plane_lib.PlaneInfo}
    mirrors = {c for c in vars(_plane_lib).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and getattr(c, "_fields_", None)}
    assert mirrors == set(pairs.values())
    consts = {"TKNN_PLANE_BATCH": _plane_lib.PLANE_BATCH, "TKNN_PLANE_OK": _plane_lib.PLANE_OK, "TKNN_PLANE_DUPLICATE": _plane_lib.PLANE_DUPLICATE,
              "TKNN_PLANE_DEGENERATE": _plane_lib.PLANE_DEGENERATE, "TKNN_PLANE_ANGLE": _plane_lib.PLANE_ANGLE}
    assert (ps.BATCH, ps.OK, ps.DUPLICATE, ps.DEGENERATE, ps.ANGLE) == tuple(consts.values()) and ps.STATUS == _plane_lib.STATUS
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn_plane.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    for cname in consts:
        lines.append('  printf("const %s %%ld\\n", (long)%s);' % (cname, cname))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = 0
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, what, value = line.split()
        if cname == "const":
            assert consts[what] == int(value), what
        elif what == "size":
            assert ctypes.sizeof(pairs[cname]) == int(value), cname
        else:
            assert getattr(pairs[cname], what).offset == int(value), (cname, what)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in pairs.values()) + len(consts)
    assert ctypes.sizeof(_plane_lib.PlaneOptions) == 88 and ctypes.sizeof(_plane_lib.PlaneInfo) == 184
    res, args = _plane_lib.SIGNATURES["tknnSegmentPlane"]
    lib = _plane_lib.load()
    assert lib is _lib.load() and lib.tknnSegmentPlane.restype is res is ctypes.c_int and lib.tknnSegmentPlane.argtypes == args
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT tknnSegmentPlane$", exported, flags=re.M), "the library exports the symbol"
