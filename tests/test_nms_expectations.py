"""tests/nms_spec.py against itself: the sequential loop's result has the properties that define the kept set, checked from a
dense matrix of the within-r predicate that the loop never builds.  No GPU."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import nms_spec as ns  # noqa: E402
from query_spec import distance32  # noqa: E402


def dist_matrix(A):
    """(m, m) float32 distances of the rows of A, 512 rows at a time."""
    out = np.empty((len(A), len(A)), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(A), 512):
            out[s:s + 512] = distance32(A[None, :, :], A[s:s + 512, None, :])
    return out


def clouds_of(c):
    P = ns.pad_to_3d(np.asarray(c["P"], np.float32))
    n = len(P)
    batch = np.zeros(n, np.int64) if c["batch"] is None else np.asarray(c["batch"], np.int64)
    B = 1 if c["batch"] is None else int(c["num_batches"])
    names = np.arange(n, dtype=np.int64) if c["ids"] is None else np.asarray(c["ids"], np.int64)
    ok = ~np.isnan(P).any(axis=1)
    if c["scores"] is not None:
        ok &= ~np.isnan(c["scores"])
    return P, batch, B, names, ok


@pytest.mark.parametrize("name", sorted(ns.CASES))
def test_the_kept_set_has_its_defining_properties(name):
    c, want = ns.case(name), ns.want(name)
    P, batch, B, names, ok = clouds_of(c)
    key = ns.keys(names, c["scores"], c["by_name"])
    keep, cover = want["keep"], want["cover"]
    assert len(np.unique(names)) == len(names) and len(np.unique(key)) == len(key)
    assert not keep[~ok].any() and (cover[~ok] == -1).all() and want["eligible"] == ok.sum()
    assert np.array_equal(cover[keep], names[keep].astype(np.int32))
    row_of = {int(v): i for i, v in enumerate(names)}
    for b in range(B):
        rows = np.flatnonzero(ok & (batch == b))
        assert want["counts"][b] == keep[rows].sum()
        if len(rows) == 0:
            continue
        d = dist_matrix(P[rows])
        near = d <= c["r"]
        k = keep[rows]
        # no two kept points of a cloud are within r
        among = near[np.ix_(k, k)]
        assert among.sum() == k.sum() and among.diagonal().all()
        # p is kept iff no kept point with a better key is within r: a dropped point has such a dominator, a kept one none
        better = key[rows][None, :] > key[rows][:, None]  # [p, q]: q beats p
        dominated = (near & better & k[None, :]).any(axis=1)
        assert np.array_equal(dominated, ~k)
        # cover: a kept point of the same cloud, within r, and none is nearer (distance bits, then name)
        for t in np.flatnonzero(~k):
            rep = row_of[int(cover[rows[t]])]
            assert keep[rep] and batch[rep] == b and ok[rep]
            j = int(np.flatnonzero(rows == rep)[0])
            assert near[t, j]
            cand = np.flatnonzero(near[t] & k)
            best = min((int(d[t, q].view(np.uint32)), int(names[rows[q]])) for q in cand)
            assert best == (int(d[t, j].view(np.uint32)), int(names[rep]))
        # the cloud alone gives the same
        alone = ns.brute(P[rows], c["r"], scores=None if c["scores"] is None else c["scores"][rows], ids=names[rows], by_name=c["by_name"])
        assert np.array_equal(alone["keep"], keep[rows]) and np.array_equal(alone["cover"], cover[rows]) and alone["counts"][0] == k.sum()


def test_fmix32_by_hand():
    # murmur3's finaliser, worked through with Python integers
    def by_hand(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        h ^= h >> 16
        return h

    assert by_hand(0) == 0 and by_hand(1) == 0x514E28B7 and by_hand(2) == 0x30F4C306 and by_hand(0xFFFFFFFF) == 0x81F16F39
    got = ns.fmix32(np.array([0, 1, 2, 0xFFFFFFFF], np.uint32))
    assert got.dtype == np.uint32 and got.tolist() == [0, 0x514E28B7, 0x30F4C306, 0x81F16F39]
    names = np.array([5, -3, 70000, 2**31 - 1, -2**31], np.int64)
    assert (ns.keys(names) >> np.uint64(32)).tolist() == [by_hand(int(v) & 0xFFFFFFFF) for v in names]


def test_key_order():
    # among equal strengths the smaller name wins, compared as int32
    k = ns.keys(np.array([-5, 0, 7, 2**31 - 1, -2**31]), by_name=True)
    assert np.argsort(k)[::-1].tolist() == [4, 0, 1, 2, 3]
    # the scores' image orders like the floats, with -0 below +0
    s = np.array([-np.inf, -3.0, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], np.float32)
    img = ns.score_image(s)
    assert (np.diff(img.astype(np.int64)) > 0).all()
    k = ns.keys(np.arange(8)[::-1].copy(), scores=s)
    assert (np.diff(k.astype(np.float64)) > 0).all(), "the strength decides before the name"


def test_line_cases():
    for name in ("line_scored", "line_by_name"):
        c, want = ns.case(name), ns.want(name)
        assert ns.max_depth(name) == ns.LINE_POINTS == 400
        along = np.argsort(c["P"][:, 0])
        kept = want["keep"][along]
        start = 0 if name == "line_by_name" else 1  # the winner is the line's first point, or its last (index 399)
        assert kept[start::2].all() and not kept[1 - start::2].any() and want["counts"][0] == 200


def test_named_outcomes():
    assert ns.want("copies")["counts"].tolist() == [1, 1]
    assert ns.want("large_r")["counts"].tolist() == [1, 1]
    assert ns.want("tiny_r")["keep"].all()
    assert ns.want("lattice_below_step")["keep"].all() and 0 < ns.want("lattice_at_step")["counts"][0] < 12 ** 3
    assert ns.want("clouds")["counts"][0] == 0 and (ns.want("clouds")["counts"][1:] > 0).all()
    z = ns.want("signed_zeros")
    assert np.flatnonzero(z["keep"]).tolist() == [1] and (z["cover"] == 1).all()
    nan = ns.want("nan")
    assert nan["bad_scores"] == 40 and nan["eligible"] < 800 - 40 and (nan["cover"][~nan["keep"]] != np.arange(800)[~nan["keep"]]).all()
    assert ns.max_depth("uniform1") == 1 and ns.max_depth("tiny_r") == 1 and ns.max_depth("large_r") > 100
