"""What the GPU tests of tknnPeriodicKnn expect (tests/periodic_spec.py), checked on the CPU: the header include/owlknn_periodic.h,
the ctypes records of owlraytracing_amd/_periodic_lib.py and the library agree; periodic_metric.h, compiled for the host, is the
spec's formula bit for bit and its box bound is a lower bound; every GPU case can catch what it is meant to catch.  Runs without
a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_spec as kn  # noqa: E402
import periodic_metric_host as pm  # noqa: E402
import periodic_spec as ps  # noqa: E402

ARG = -1
CELLS = (ps.UNIT, ps.CELL)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the header, the binding, the library -------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"TKNN_API[^;(]*?\b(tknn\w+)\s*\(", text))


def test_header_binding_and_struct_layouts_agree(tmp_path):
    """tknnPeriodicKnn is declared in its own header, exported and bound with its signature, nothing was added to owlknn.h,
    owlknn_knn.h or their tables, and the ctypes records have the header's sizes and offsets (gcc, C99)."""
    from owlraytracing_amd import _knn_lib, _lib, _periodic_lib

    assert _declared("owlknn_periodic.h") == set(_periodic_lib.SIGNATURES) == {"tknnPeriodicKnn"}
    for header, table in (("owlknn.h", _lib.SIGNATURES), ("owlknn_knn.h", _knn_lib.SIGNATURES)):
        assert "tknnPeriodicKnn" not in _declared(header) and "tknnPeriodicKnn" not in table
    assert not hasattr(_lib, "PeriodicKnnOptions") and not hasattr(_knn_lib, "PeriodicKnnOptions")
    res, args = _periodic_lib.SIGNATURES["tknnPeriodicKnn"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.POINTER(_periodic_lib.PeriodicKnnOptions),
                                            ctypes.POINTER(_periodic_lib.PeriodicKnnInfo), ctypes.c_void_p]
    pairs = {"tknnPeriodicKnnOptions": _periodic_lib.PeriodicKnnOptions, "tknnPeriodicKnnInfo": _periodic_lib.PeriodicKnnInfo}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn_periodic.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        cname, what, value = line.split()
        cls = pairs[cname]
        if what == "size":
            assert ctypes.sizeof(cls) == int(value), cname
        else:
            assert getattr(cls, what).offset == int(value), (cname, what)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in pairs.values())
    assert ctypes.sizeof(_periodic_lib.PeriodicKnnOptions) == 88 and ctypes.sizeof(_periodic_lib.PeriodicKnnInfo) == 72
    assert [f for f, _ in _periodic_lib.PeriodicKnnInfo._fields_] == [f for f, _ in _knn_lib.KnnInfo._fields_], "as tknnKnnInfo counts them"
    lib = _periodic_lib.load()
    assert lib is _lib.load() and lib.tknnPeriodicKnn.restype is ctypes.c_int and lib.tknnPeriodicKnn.argtypes == args
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT tknnPeriodicKnn$", exported, flags=re.M), "the library exports the symbol"
    for name in ("periodic_knn.hip", "periodic_metric.h", "owlknn_periodic.h"):
        assert all(name in v for v in _lib._NOT_IN.values()), "the per-kernel profile records of team_* and db_* do not depend on it"


def test_a_null_engine_is_refused_without_a_device():
    from owlraytracing_amd import _periodic_lib

    lib = _periodic_lib.load()
    o, info = _periodic_lib.PeriodicKnnOptions(), _periodic_lib.PeriodicKnnInfo()
    info.total = 99
    assert lib.tknnPeriodicKnn(None, ctypes.byref(o), ctypes.byref(info), None) == ARG
    text = lib.tknnLastError().decode()
    assert text.startswith("tknnPeriodicKnn: ") and "engine" in text and info.total == 99, text


# ---- periodic_metric.h on the host --------------------------------------------------------------------------------------------------
def _largest_in_cell(lo, L):
    """The largest float x with fl(x - lo) <= L (a periodic axis)."""
    x = np.float32(lo + L)
    while np.float32(x - lo) <= L:
        x = np.nextafter(x, np.float32(np.inf))
    while not np.float32(x - lo) <= L:
        x = np.nextafter(x, np.float32(-np.inf))
    return x


def _snap_into_cell(X, lo, period):
    """X with every coordinate of a periodic axis moved to the nearest in-cell value."""
    X = np.array(X, np.float32)
    for t in range(3):
        if period[t] > 0:
            top = _largest_in_cell(lo[t], period[t])
            X[:, t] = np.minimum(np.maximum(X[:, t], lo[t]), top)
    assert ps.in_cell(X, lo, period).all()
    return X


def test_in_cell_is_the_specs():
    for lo, period in CELLS:
        for t in range(3):
            if not period[t] > 0:
                continue
            hi = np.float32(lo[t] + period[t])
            x = np.float32([lo[t], np.nextafter(lo[t], np.float32(-9)), np.nextafter(lo[t], np.float32(9)), hi, np.nextafter(hi, np.float32(9)),
                            np.nextafter(hi, np.float32(-9)), _largest_in_cell(lo[t], period[t]), np.nan, np.inf, -np.inf, 0, 1e30])
            X = np.tile(lo + period / 2, (len(x), 1)).astype(np.float32)
            X[:, t] = x
            assert np.array_equal(pm.in_cell(x, lo[t], period[t]), ps.in_cell(X, lo, period)), (lo, period, t)
    assert pm.in_cell(np.float32([np.nan, 5, -np.inf]), 0.0, 0.0).all(), "an open axis holds everything"


def test_periodic_dist2_is_the_specs_formula_bit_for_bit():
    rng = np.random.default_rng(92)
    n = 200_000
    for lo, period in CELLS + ((np.float32([0, 0, 0]), np.float32([0, 0, 0])), (np.float32([-3, 5, 100]), np.float32([0.37, 0, 1e-3]))):
        width = np.where(period > 0, period, np.float32(1)).astype(np.float32)
        P = (lo + rng.random((n, 3), dtype=np.float32) * width).astype(np.float32)
        Q = (lo + rng.random((n, 3), dtype=np.float32) * width).astype(np.float32)
        Q[: n // 4] = P[: n // 4] + (rng.random((n // 4, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(1e-5)  # close pairs
        Q[n // 4: n // 2] = P[n // 4: n // 2] + period * np.float32(0.5)  # pairs half a period apart, where the two branches meet
        P[::97, 0], Q[::89, 1], P[::83, 2] = np.nan, np.nan, np.inf
        with np.errstate(invalid="ignore", over="ignore"):
            a = np.abs(P - Q)
            w = [np.minimum(a[:, t], np.abs(period[t] - a[:, t])) if period[t] > 0 else a[:, t] for t in range(3)]
            d2 = ((w[0] * w[0]) + (w[1] * w[1])) + (w[2] * w[2])
        assert d2.dtype == np.float32
        got = pm.dist2(P, Q, lo, period)
        both_nan = np.isnan(got) & np.isnan(d2)
        assert np.array_equal(_bits(got)[~both_nan], _bits(d2)[~both_nan]) and (np.isnan(got) == np.isnan(d2)).all(), (lo, period)
        assert np.isnan(got[::97]).all() and np.isnan(got[::89]).all(), "fminf must not swallow the NaN"
        # the pairwise form the brute force uses is the same numbers
        assert np.array_equal(_bits(np.sqrt(d2[:64], dtype=np.float32)), _bits(np.diagonal(ps.wrapped(P[:64], Q[:64], lo, period))))
    # with no periodic axis: knn_dist2, through the open-space spec
    P, Q = rng.random((500, 3), dtype=np.float32), rng.random((40, 3), dtype=np.float32)
    open_rows = kn.knn_rows(P, Q, 9)
    for lo, period in ((np.zeros(3, np.float32), np.zeros(3, np.float32)), (np.float32([-4.5, -4.5, -4.5]), np.float32([10, 10, 10]))):
        rows = ps.knn_rows(P, Q, 9, lo, period)
        assert all(np.array_equal(_bits(rows[key]) if key == "dist" else rows[key], _bits(open_rows[key]) if key == "dist" else open_rows[key])
                   for key in rows), "no periodic axis, or a cell ten scene widths wide: the open rows"


def _bound_triples(lo, period, rng, boxes, per_box):
    """(blo, bhi, p, q), `boxes * per_box` rows each: boxes anywhere near the cell, touching and straddling its faces included; p the
    in-cell points of a box (corners, face points, interior); q in the cell -- anywhere, within an ulp of lo and of lo + L, and
    within a few ulps of a box face or of its image a period away (where an ulp of slack decides)."""
    width = np.where(period > 0, period, np.float32(1)).astype(np.float32)
    scale = np.float32(10.0) ** -rng.integers(0, 7, (boxes, 1)).astype(np.float32)  # extents from the cell's width down to 1e-6 of it
    a = lo + (rng.random((boxes, 3), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)) * width
    b = a + rng.random((boxes, 3), dtype=np.float32) * width * scale
    kind = rng.integers(0, 4, (boxes, 3))
    top = np.float32([_largest_in_cell(lo[t], period[t]) if period[t] > 0 else 0 for t in range(3)])
    a = np.where(kind == 1, lo, a).astype(np.float32)  # touches the lower face
    b = np.where((kind == 2) & (period > 0), top, b).astype(np.float32)  # touches the upper face
    a = np.minimum(a, b).astype(np.float32)
    blo, bhi = np.repeat(a, per_box, axis=0), np.repeat(b, per_box, axis=0)
    n = len(blo)
    # p: in the box and in the cell
    u = rng.random((n, 3), dtype=np.float32)
    pick = rng.integers(0, 3, (n, 3))
    p = np.where(pick == 0, blo, np.where(pick == 1, bhi, blo + u * (bhi - blo))).astype(np.float32)
    p = np.minimum(np.maximum(p, blo), bhi)
    p_in = _snap_into_cell(p, lo, period)
    ok = ((p_in >= blo) & (p_in <= bhi)).all(axis=1)  # (a box wholly outside the cell has no in-cell point: dropped)
    # q: in the cell
    q = (lo + rng.random((n, 3), dtype=np.float32) * width).astype(np.float32)
    qk = rng.integers(0, 8, (n, 3))
    steps = rng.integers(-3, 4, (n, 3))
    near = np.where(rng.integers(0, 2, (n, 3)) == 0, blo, bhi).astype(np.float32)
    image = np.where(qk == 3, near - period, np.where(qk == 4, near + period, near)).astype(np.float32)
    for _ in range(3):  # up to three ulps to either side
        image = np.where(steps > 0, np.nextafter(image, np.float32(np.inf)), np.where(steps < 0, np.nextafter(image, np.float32(-np.inf)), image))
        steps = steps - np.sign(steps)
    q = np.where((qk >= 3) & (qk <= 5), image, q).astype(np.float32)
    q = np.where(qk == 6, np.where(steps == 0, lo, np.nextafter(lo, np.float32(np.inf))), q).astype(np.float32)
    q = np.where((qk == 7) & (period > 0), np.where(u < 0.5, top, np.nextafter(top, np.float32(-np.inf))), q).astype(np.float32)
    q = _snap_into_cell(q, lo, period)
    return blo[ok], bhi[ok], p_in[ok], q[ok]


def test_the_box_bound_is_a_lower_bound():
    """periodic_box_min_dist2(box, q) * 0.999995f <= periodic_dist2(p, q) for every in-cell p of the box, the way beyond_gate uses
    it -- over more than 10^6 seeded triples per cell.  This is where a missing ulp of slack shows; random GPU rows do not find it."""
    rng = np.random.default_rng(93)
    for lo, period in CELLS + ((np.float32([100.1, -300.3, 0]), np.float32([0.3, 0.7, 0.001])),):
        blo, bhi, p, q = _bound_triples(lo, period, rng, 48_000, 32)
        assert len(p) >= 1_000_000, len(p)
        bound = pm.box_min_dist2(blo, bhi, q, lo, period)
        d2 = pm.dist2(p, q, lo, period)
        assert np.isfinite(bound).all() and np.isfinite(d2).all()
        bad = np.flatnonzero(~(bound * np.float32(0.999995) <= d2))
        assert not len(bad), "%d of %d triples: e.g. box %s .. %s, p %s, q %s: bound %g > d2 %g" % (
            len(bad), len(p), blo[bad[0]], bhi[bad[0]], p[bad[0]], q[bad[0]], bound[bad[0]], d2[bad[0]])
        assert (bound <= d2).all(), "periodic_metric.h derives more: the bound holds without the factor"
        # the triples are sharp: many bounds are positive, many pairs are nearest across a face, many queries sit at a face
        crosses = _bits(d2) != _bits(pm.dist2(p, q, lo, np.zeros(3, np.float32)))
        assert (bound > 0).mean() > 0.3 and crosses.mean() > 0.2, ((bound > 0).mean(), crosses.mean())
        tight = (bound > 0) & (bound >= d2 * np.float32(0.99))
        assert tight.sum() > 1000, "bounds within a percent of the distance they bound: %d" % tight.sum()
    # no periodic axis: box_min_dist2 of team_walk.h, the plain gaps
    zero = np.zeros(3, np.float32)
    blo, bhi, p, q = _bound_triples(ps.UNIT[0], ps.UNIT[1], rng, 2000, 8)
    g = np.maximum(np.maximum(blo - q, q - bhi), np.float32(0))
    assert np.array_equal(_bits(pm.box_min_dist2(blo, bhi, q, zero, zero)), _bits(((g[:, 0] * g[:, 0]) + (g[:, 1] * g[:, 1])) + (g[:, 2] * g[:, 2])))


# ---- the GPU cases are sharp ----------------------------------------------------------------------------------------------------------
def _crossing(P, Q, lo, period, idx):
    """Per entry of idx (m, k): its wrapped distance differs from its open distance (padding: False)."""
    d = ps.wrapped(P, Q, lo, period).view(np.int32) != ps.wrapped(P, Q, lo, period, wrap=False).view(np.int32)
    return np.take_along_axis(d, np.maximum(idx, 0).astype(np.int64), axis=1) & (idx >= 0)


def test_the_uniform_case_crosses_faces():
    """Measured here: 48 % of the external rows of k = 32 hold an entry nearest across a face and 17 % have one at the k-th place
    (the set's own rows: 45 % and 15 %); at k = 16, 35 % and 10 %."""
    P, Q, lo, period = ps.uniform_case()
    assert len(P) == 2000 and len(Q) == 300 and ps.in_cell(P, lo, period).all() and ps.in_cell(Q, lo, period).all()
    for name, queries, rows in (("external", Q, ps.knn_rows(P, Q, 32, lo, period)), ("self", P, ps.self_rows(P, 32, lo, period))):
        c = _crossing(P, queries, lo, period, rows["idx"])
        print("%s: %.0f %% of the rows cross a face, %.0f %% at the k-th place" % (name, 100 * c.any(axis=1).mean(), 100 * c[:, -1].mean()))
        assert c.any(axis=1).mean() >= 0.30 and c[:, -1].mean() >= 0.10, name
        assert c[:, :16].any(axis=1).mean() >= 0.30, name
    open_rows = kn.knn_rows(P, Q, 32)
    assert (open_rows["idx"] != ps.knn_rows(P, Q, 32, lo, period)["idx"]).any(axis=1).mean() >= 0.30, "an open-space answer fails the case"


def test_the_lattice_case_crosses_faces_and_ties():
    P, Q, face = ps.lattice_case()
    lo, period = ps.UNIT
    assert len(P) == 4096 and len(face) == 256 and ps.in_cell(Q, lo, period).all()
    kmax = max(ps.LATTICE_K)
    rows, own = ps.knn_rows(P, Q, kmax + 1, lo, period), ps.self_rows(P, kmax + 1, lo, period)
    assert _crossing(P, Q, lo, period, rows["idx"][:, :kmax]).any(axis=1).all(), "every chosen query's row crosses a face"
    assert _crossing(P, P, lo, period, own["idx"][:, :kmax])[face].any(axis=1).all(), "every row of the x = 0 face crosses it"
    d, od = rows["dist"].view(np.int32), own["dist"].view(np.int32)
    for k in ps.LATTICE_K:
        assert (d[:, k - 1] == d[:, k]).any(), "external ties at the k-th place, k = %d" % k
    for k in (1, 3, 7):
        assert (od[face, k - 1] == od[face, k]).all(), "self-mode ties at the k-th place, k = %d" % k
    # a radius of exactly the spacing: six neighbours exactly at r in every row, three of them across a face for the corner point
    r = ps.LATTICE_SPACING
    at_r = ps.self_rows(P, 7, lo, period, radius=r)
    assert (at_r["counts"] == 6).all() and (at_r["dist"][:, :6] == r).all()
    corner = int(np.flatnonzero((P == 0).all(axis=1))[0])
    assert _crossing(P, P[corner:corner + 1], lo, period, at_r["idx"][corner:corner + 1]).sum() == 3


def test_the_tiny_case_goes_beyond_half_a_period():
    lo, period = ps.UNIT
    for n in ps.TINY_N:
        P, Q, ks = ps.tiny_case(n)
        assert len(P) == n and min(ks) <= n and max(ks) > n or n > ps.K_MAX
        assert ks[0] < n or n == 1
        rows = ps.knn_rows(P, Q, ps.K_MAX, lo, period)
        assert (rows["counts"] == min(n, ps.K_MAX)).all()
        with np.errstate(invalid="ignore"):
            assert ((rows["dist"] > 0.5) & np.isfinite(rows["dist"])).any(axis=1).all(), "every row has an entry beyond half a period"
        s = np.sort(rows["idx"], axis=1)
        assert not ((s[:, 1:] == s[:, :-1]) & (s[:, 1:] >= 0)).any(), "no row has a duplicate"
        if n <= ps.K_MAX:
            assert all((np.sort(row[:n]) == np.arange(n)).all() for row in rows["idx"]), "each point exactly once"


def test_the_edge_case_has_every_kind_of_row():
    P, Q, radii = ps.edge_case()
    lo, period = ps.CELL
    inside = ps.in_cell(Q, lo, period)
    assert (~inside[[1, 2, 3, 4, 7, 8]]).all() and inside[[0, 5, 6, 10]].all() and inside[9], "a NaN on the open axis is no matter of the cell"
    rows = ps.knn_rows(P, Q, 64, lo, period)
    assert (rows["counts"][[1, 2, 3, 4, 7, 8, 9]] == 0).all() and (rows["counts"][[0, 5, 6, 10]] == 64).all()
    assert rows["dist"][0, 39] == 0 and rows["dist"][0, 40] > 0, "40 copies of the query: a seed bound of 0 up to k = 40"
    nan_p = np.flatnonzero(np.isnan(P).any(axis=1))
    assert len(nan_p) == 20 and not np.isin(rows["idx"], nan_p).any()
    with_r = ps.knn_rows(P, Q, 64, lo, period, radii=radii)
    assert (with_r["counts"][11:16] == 0).all() and with_r["counts"][16] == 64 and with_r["counts"][17] == 0
    assert (with_r["counts"][18:] > 0).all() and (with_r["counts"][18:] < 64).any()


def test_the_pyramid_case_has_three_levels():
    P, Q = ps.pyramid_case()
    blocks = -(-len(P) // 16)
    assert 64 * 64 < blocks <= 64 ** 3, "blocks, 64 times fewer nodes, at most 64 of them under the root's level"
    lo, period = ps.UNIT
    near = np.minimum(Q - lo, lo + period - Q).min(axis=1)
    assert (near[:128] <= 0.0101).all() and len(Q) == 256
