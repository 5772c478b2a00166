"""What the tests of the batched build and of TrueKNN.batch_knn rest on, checked without a GPU: tests/batch_spec.py against
scipy's cKDTree per batch, the batched key through the host-compiled curve_key.h, the bits the labels take, and the header,
the binding and the library's exports."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_spec as bs  # noqa: E402
import curve_key_host  # noqa: E402
import knn_spec as kn  # noqa: E402

ARG = -1


# ---- the spec ------------------------------------------------------------------------------------------------------------------------
def test_the_spec_is_a_kd_tree_per_batch():
    """On distinct distances row j is cKDTree(P[batch == b_j]).query(q_j, k), the indices mapped back, and a label without
    points gives an empty row."""
    from scipy.spatial import cKDTree

    P, batch, Q, batch_q = bs.clouds_case()
    k = 10
    rows = bs.knn_rows(P, batch, Q, batch_q, k)
    for b in range(len(bs.CLOUD_SIZES)):
        members = np.flatnonzero(batch == b)
        mine = np.flatnonzero(batch_q == b)
        assert len(members) == bs.CLOUD_SIZES[b] and len(mine) == 30
        want = min(k, len(members))
        assert (rows["counts"][mine] == want).all()
        assert (rows["idx"][mine, want:] == -1).all() and np.isinf(rows["dist"][mine, want:]).all()
        if not want:
            continue
        d, i = cKDTree(P[members].astype(np.float64)).query(Q[mine].astype(np.float64), k=want)
        d, i = d.reshape(len(mine), want), i.reshape(len(mine), want)
        assert (np.diff(d, axis=1) > 0).all(), "distinct distances: the order is the distance's alone"
        assert np.array_equal(members[i], rows["idx"][mine, :want])
        assert np.allclose(d, rows["dist"][mine, :want], rtol=1e-6, atol=0)
        assert (batch[rows["idx"][mine, :want]] == b).all()


def test_the_spec_is_knn_spec_with_one_label():
    """One batch: tests/knn_spec.py's rows, bit for bit -- external, with skips and ids, and the set's own points."""
    P, Q = kn.nan_case()
    zeros_p, zeros_q = np.zeros(len(P), np.int32), np.zeros(len(Q), np.int32)
    ids = (np.arange(len(P), dtype=np.int32) * 7 + 3)[::-1].copy()
    skip = np.where(np.arange(len(Q)) % 2, -1, ids[np.arange(len(Q)) * 5 % len(P)])
    for k in (1, 17):
        for a, b in ((bs.knn_rows(P, zeros_p, Q, zeros_q, k), kn.knn_rows(P, Q, k)),
                     (bs.knn_rows(P, zeros_p, Q, zeros_q, k, skip=skip, ids=ids), kn.knn_rows(P, Q, k, skip=skip, ids=ids)),
                     (bs.self_rows(P, zeros_p, k), kn.self_rows(P, k)), (bs.self_rows(P, zeros_p, k, ids=ids), kn.self_rows(P, k, ids=ids))):
            assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["counts"], b["counts"])
            assert np.array_equal(a["dist"].view(np.int32), b["dist"].view(np.int32))


def test_radii_skips_and_labels_of_the_spec():
    P, batch, Q, batch_q, radii = bs.nan_case()
    rows = bs.knn_rows(P, batch, Q, batch_q, 64, radii=radii)
    assert (rows["counts"][[0, 7, 8, 9]] == 0).all(), "a NaN, infinite, zero or negative radius: an empty row"
    assert (rows["counts"][[1, 20, 41, 62]] == 0).all(), "a label no batch has: an empty row"
    assert (rows["counts"][[3, 17, 18, 40, 63]] == 0).all(), "a NaN query: an empty row"
    assert rows["counts"][33] == 64 and rows["counts"].max() == 64 and (rows["counts"] > 0).sum() > 30
    filled = rows["idx"] >= 0
    assert (batch[rows["idx"][filled]] == np.broadcast_to(batch_q[:, None], rows["idx"].shape)[filled]).all()
    assert (rows["dist"][filled] <= np.broadcast_to(radii[:, None], rows["idx"].shape)[filled]).all()
    assert not np.isnan(P[rows["idx"][filled]]).any()
    free = bs.knn_rows(P, batch, Q, batch_q, 3)
    skipped = bs.knn_rows(P, batch, Q, batch_q, 3, skip=free["idx"][:, 0])
    ok = free["counts"] == 3
    assert np.array_equal(skipped["idx"][ok, 0], free["idx"][ok, 1])
    own = bs.self_rows(P, batch, 5)
    assert not (own["idx"] == np.arange(len(P))[:, None]).any()
    assert (own["counts"][np.isnan(P).any(axis=1)] == 0).all()
    TP, tb, TQ, tq = bs.twins_case()
    twins = bs.knn_rows(TP, tb, TQ, tq, 2)
    assert (twins["dist"][:80, 0] == 0).all() and (twins["dist"][:80, 1] > 0).all() and (twins["dist"][80:, 0] > 0).all()
    assert (tb[twins["idx"][:40, 0]] == 0).all() and (tb[twins["idx"][40:80, 0]] == 1).all()
    town = bs.self_rows(TP, tb, 1)
    assert (town["dist"][tb < 2, 0] > 0).all(), "the twin in the other batch is no neighbour"


# ---- the key ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_batches,bits", [(1, 0), (2, 3), (8, 3), (9, 6), (64, 6), (65, 9), (32768, 15)])
def test_key_bits(num_batches, bits):
    from owlraytracing_amd import _batch_lib

    assert bs.key_bits(num_batches) == _batch_lib.key_bits(num_batches) == bits
    assert bits % 3 == 0 and 2 ** bits >= num_batches and (bits == 0 or 2 ** (bits - 3) < num_batches)
    assert bs.MAX_BATCHES == _batch_lib.MAX_BATCHES == 32768


@pytest.mark.parametrize("curve", [curve_key_host.HILBERT, curve_key_host.MORTON])
@pytest.mark.parametrize("num_batches", [1, 7, 33, 4096, 32768])
def test_the_batched_key_groups_the_labels_in_curve_order(num_batches, curve):
    """A stable sort by the batched key groups the labels, ascending; inside a label it is the stable order of key21 >> bb,
    which is the key of the point's cell at level 21 - bb / 3 of the same grid (the hierarchy of curve_key.h) and NOT the key
    curve_point_key gives at that many levels; NaN points come last in input order; one batch leaves the keys as they are."""
    lib = curve_key_host.load()
    rng = np.random.default_rng(350 + num_batches)
    n = 5000
    P = (rng.random((n, 3), dtype=np.float32) * np.float32(3.7) - np.float32(1.3)).astype(np.float32)
    P[rng.choice(n, 11, replace=False), 1] = np.nan
    labels = rng.integers(0, num_batches, n)
    clean = ~np.isnan(P).any(axis=1)
    lo = P[clean].min(0)
    ext = np.float32((P[clean].max(0) - lo).max())
    key21 = curve_key_host.point_keys(lib, curve, 21, P, lo, ext)
    keys = bs.batched_keys(key21, labels, num_batches)
    bb = bs.key_bits(num_batches)
    assert np.array_equal(keys[~clean], np.full(11, 1 << 63, np.uint64)) and (keys[clean] >> np.uint64(63) == 0).all()
    assert np.array_equal(keys[clean] >> np.uint64(63 - bb), labels[clean].astype(np.uint64))
    if num_batches == 1:
        assert np.array_equal(keys, key21)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(order[-11:], np.flatnonzero(~clean))
    head = order[:-11]
    assert (np.diff(labels[head]) >= 0).all(), "the labels are grouped, ascending"
    want = np.lexsort((np.arange(n)[clean], key21[clean] >> np.uint64(bb), labels[clean]))
    assert np.array_equal(head, np.flatnonzero(clean)[want])
    # key21 >> bb is the level-(21 - bb / 3) key of the point's cell
    levels = 21 - bb // 3
    cells = (1 << 21) - 1
    with np.errstate(invalid="ignore"):
        q = np.clip((P[clean] - lo) * (np.float32(cells) / ext), 0, np.float32(cells)).astype(np.uint32)
    assert np.array_equal(curve_key_host.keys(lib, curve, 21, q[:, 0], q[:, 1], q[:, 2]), key21[clean])
    up = np.uint32(21 - levels)
    assert np.array_equal(curve_key_host.keys(lib, curve, levels, q[:, 0] >> up, q[:, 1] >> up, q[:, 2] >> up), key21[clean] >> np.uint64(bb))
    if bb:
        assert not np.array_equal(curve_key_host.point_keys(lib, curve, levels, P[clean], lo, ext), key21[clean] >> np.uint64(bb)), \
            "requantised keys differ: their scale is 2^levels - 1 cells, not 2^21 - 1"


def test_the_build_spec_with_one_batch_is_lbvh_spec():
    import lbvh_spec as ls

    P, _ = bs.build_case(7)
    got, want = bs.build_points(P, np.zeros(len(P), np.int32), 1), ls.build_points(P)
    assert not ls.compare(got, want)
    assert got["starts"].tolist() == [0, len(P) - 9]
    P, batch = bs.build_case(33)
    got = bs.build_points(P, batch, 33)
    assert got["starts"][0] == 0 and got["starts"][-1] == len(P) - 9 and got["starts"][2] == got["starts"][3], "batch 2 is empty"
    assert np.array_equal(np.diff(got["starts"]), np.bincount(batch[~np.isnan(P).any(axis=1)], minlength=33))
    assert (batch[got["prim_id"][:len(P) - 9]] == np.repeat(np.arange(33), np.diff(got["starts"]))).all()


# ---- the header, the binding, the library -------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"TKNN_API[^;(]*?\b(tknn\w+)\s*\(", text))


def test_header_binding_and_struct_layouts_agree(tmp_path):
    """The three entry points are declared in their own header (strict C99), exported and bound with their signatures, nothing
    was added to the other headers or their tables, and the ctypes records have the header's sizes and offsets."""
    from owlraytracing_amd import _batch_lib, _knn_lib, _lib, _periodic_lib

    names = {"tknnBuildBatched", "tknnBatchLayout", "tknnBatchKnn"}
    assert _declared("owlknn_batch.h") == set(_batch_lib.SIGNATURES) == names
    for header, table in (("owlknn.h", _lib.SIGNATURES), ("owlknn_knn.h", _knn_lib.SIGNATURES), ("owlknn_periodic.h", _periodic_lib.SIGNATURES)):
        assert not names & _declared(header) and not names & set(table)
    pairs = {"tknnBatchKnnOptions": _batch_lib.BatchKnnOptions, "tknnBatchKnnInfo": _batch_lib.BatchKnnInfo}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn_batch.h"', "int main(void) {",
             '  printf("max batches %d\\n", TKNN_MAX_BATCHES);']
    for cname, cls in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "max batches %d" % _batch_lib.MAX_BATCHES
    seen = 0
    for line in out[1:]:
        cname, what, value = line.split()
        cls = pairs[cname]
        if what == "size":
            assert ctypes.sizeof(cls) == int(value), cname
        else:
            assert getattr(cls, what).offset == int(value), (cname, what)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in pairs.values())
    assert ctypes.sizeof(_batch_lib.BatchKnnOptions) == 72 and ctypes.sizeof(_batch_lib.BatchKnnInfo) == 72
    assert [f for f, _ in _batch_lib.BatchKnnInfo._fields_] == [f for f, _ in _knn_lib.KnnInfo._fields_], "tknnKnnInfo's fields"
    want = [f for f, _ in _periodic_lib.PeriodicKnnOptions._fields_ if f not in ("lo", "period")]
    want.insert(want.index("d_skip_ids") + 1, "d_query_batch")
    assert [f for f, _ in _batch_lib.BatchKnnOptions._fields_] == want, "tknnPeriodicKnnOptions without the cell, plus the labels"
    lib = _batch_lib.load()
    assert lib is _lib.load()
    for name, (res, args) in _batch_lib.SIGNATURES.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in names:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), "the library exports %s" % name
    for name in ("batch_knn.hip", "owlknn_batch.h"):
        assert all(name in v for v in _lib._NOT_IN.values()), "the per-kernel profile records of team_* and db_* do not depend on it"


def test_a_null_engine_is_refused_without_a_device():
    from owlraytracing_amd import _batch_lib, _lib

    lib = _batch_lib.load()
    o, info, binfo = _batch_lib.BatchKnnOptions(), _batch_lib.BatchKnnInfo(), _lib.BuildInfo()
    info.total, binfo.n = 99, 99
    assert lib.tknnBatchKnn(None, ctypes.byref(o), ctypes.byref(info), None) == ARG
    text = lib.tknnLastError().decode()
    assert text.startswith("tknnBatchKnn: ") and "engine" in text and info.total == 99, text
    assert lib.tknnBuildBatched(None, None, None, None, 1, 1, ctypes.byref(binfo), None) == ARG
    assert lib.tknnLastError().decode().startswith("tknnBuildBatched: ") and binfo.n == 99
    nb = ctypes.c_int32(-7)
    assert lib.tknnBatchLayout(None, ctypes.byref(nb), None, None, None) == ARG and nb.value == -7
    assert lib.tknnLastError().decode().startswith("tknnBatchLayout: ")
