"""TrueKNN.radius_reduce (tknnRadiusReduce, include/owlknn_reduce.h) against tests/reduce_spec.py: counts exactly, weight sums and
weighted value sums inside the derived tolerance, through the team walk and through the lane kernel, on the smallest shapes at
which each mechanism can go wrong -- the leaf block edge, every pyramid level, every channel tier, boxes inside the sphere (more
than a team's range list holds; the top boxes), rows of the chunk lengths, distances exactly r, NaN on either side, ids, batches."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import reduce_spec as rd  # noqa: E402

pytestmark = pytest.mark.gpu

FALLBACK = "TKNN_REDUCE_FORCE_FALLBACK"
SPEC_CHANNELS = {"n66000": 4}  # value columns the spec sums on the sets with long rows (the others: all 16)


@pytest.fixture(scope="module")
def eng():
    from owlraytracing_amd.trueknn import TrueKNN

    e = TrueKNN(device=0)
    yield e
    e.close()


def build(eng, c):
    eng.build(c["P"], ids=c["ids"], batch=c["batch"], num_batches=c["num_batches"])


def reduce(eng, P_values, Q, r, weight, C, mode="ext", normalize=False, **kw):
    """One call, its tensors as numpy."""
    res = eng.radius_reduce(r, queries=Q if mode == "ext" else None, values=None if C == 0 else np.ascontiguousarray(P_values[:, :C]), weight=weight,
                            bandwidth=rd.bandwidth(r), normalize=normalize, skip_self=mode == "own_skip", **kw)
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def check(got, want, weight, r, m, normalize=False, fallback=False):
    C = 0 if got["out"] is None else got["out"].shape[1]
    rd.compare(got, want, weight, r, rd.bandwidth(r), normalize=normalize, channels=C)
    info = got["info"]
    assert info["total"] == want["counts"].sum() and info["max_row"] == (want["counts"].max() if m else 0)
    assert not fallback or info["fallback_items"] == m, "with the fallback forced every query is the lane kernel's"
    assert info["solve_ms"] > 0 and info["walk_ms"] > 0 and (info["stage_ms"] > 0) == (C > 0)


def want_for(name, label, mode, weight):
    c = rd.case(name)
    key = ("gpu_want", name, label, mode, weight)
    if key not in rd._cache:
        r = c["radii"][label]
        rd._cache[key] = rd.sums(rd.rows_of(name, label, mode), c["values"][:, :SPEC_CHANNELS.get(name, rd.MAX_CHANNELS)], weight, r, rd.bandwidth(r))
    return rd._cache[key]


MODE_CHANNELS = {"ext": (3, False), "own": (8, True), "own_skip": (5, False)}  # channels and normalize of the call each mode makes


@pytest.mark.parametrize("weight", rd.WEIGHTS)
@pytest.mark.parametrize("name", rd.SET_NAMES)
def test_every_set_radius_class_and_mode(eng, name, weight, monkeypatch):
    c = rd.case(name)
    build(eng, c)
    for fallback in (False, True):
        if fallback:
            monkeypatch.setenv(FALLBACK, "1")
        for label, r in c["radii"].items():
            for mode in rd.modes_of(name):
                want = want_for(name, label, mode, weight)
                m = len(want["len"])
                C, normalize = MODE_CHANNELS[mode]
                got = reduce(eng, c["values"], c["Q"], r, weight, C, mode, normalize)
                check(got, want, weight, r, m, normalize, fallback)
                if mode == "own_skip":  # the count-only call: boxes inside the sphere are added arithmetically, the own slot taken out
                    bare = reduce(eng, c["values"], c["Q"], r, weight, 0, mode)
                    assert bare["out"] is None
                    check(bare, want, weight, r, m, False, fallback)
                if label == "empty" and not normalize:
                    again = reduce(eng, c["values"], c["Q"], r, weight, C, mode, True)
                    assert (again["out"][want["len"] == 0] == 0).all() and not np.signbit(again["out"][want["len"] == 0]).any()


@pytest.mark.parametrize("weight", rd.WEIGHTS)
@pytest.mark.parametrize("C", rd.CHANNEL_COUNTS)
def test_channel_tiers(eng, C, weight, monkeypatch):
    c = rd.case("n1025")
    build(eng, c)
    for fallback in (False, True):
        if fallback:
            monkeypatch.setenv(FALLBACK, "1")
        for label in ("mid", "all"):
            r = c["radii"][label]
            for mode in ("ext", "own_skip"):
                want = want_for("n1025", label, mode, weight)
                for normalize in (False, True):
                    got = reduce(eng, c["values"], c["Q"], r, weight, C, mode, normalize)
                    assert (got["out"] is None) == (C == 0)
                    check(got, want, weight, r, len(want["len"]), normalize, fallback)


def test_rows_of_the_chunk_lengths(eng, monkeypatch):
    P, Q, picks, values = rd.chunk_case()
    eng.build(P)
    for L, j, r in picks:
        mem = rd.members(P, Q, r)
        assert mem["lengths"][j] == L
        for weight in ("gauss", "cubic_spline"):
            want = rd.sums(mem, values[:, :4], weight, r, rd.bandwidth(r))
            for fallback in ("0", "1"):
                monkeypatch.setenv(FALLBACK, fallback)
                got = reduce(eng, values, Q, r, weight, 4)
                assert got["counts"][j] == L
                check(got, want, weight, r, len(Q), False, fallback == "1")


def test_distance_exactly_r_is_inside(eng, monkeypatch):
    P, Q, radii, values = rd.lattice_case()
    eng.build(P)
    lengths = []
    for r in radii:
        mem = rd.members(P, Q, r)
        lengths.append(mem["lengths"])
        for weight, C in (("one", 0), ("epanechnikov", 1), ("cubic_spline", 3), ("gauss", 5)):
            want = rd.sums(mem, values[:, :C] if C else None, weight, r, rd.bandwidth(r))
            for fallback in ("0", "1"):
                monkeypatch.setenv(FALLBACK, fallback)
                check(reduce(eng, values, Q, r, weight, C), want, weight, r, len(Q), False, fallback == "1")
    assert (lengths[0] > lengths[1]).any(), "the float below the spacing loses the neighbours at distance exactly r"


def test_values_of_other_points_never_reach_a_sum(eng, monkeypatch):
    """The leak test: every point that is no neighbour of any query holds NaN / +inf / -inf; all outputs stay finite and inside
    the tolerance -- at a radius with boxes inside the sphere (streamed ranges), at a small one, with the last partial block."""
    Q = (np.random.default_rng(61).random((5, 3), dtype=np.float32) * np.float32(0.3)).astype(np.float32)  # near one corner
    poison = np.array([np.nan, np.inf, -np.inf], np.float32)
    # 1 025 points end in a block of one point; the queries' rows on 66 000 points hold whole boxes of 1 024 and more
    for name, label, longest in (("n1025", "mid", 1), ("n66000", "half", 4096)):
        c = rd.case(name)
        build(eng, c)
        r = c["radii"][label]
        mem = rd.members(c["P"], Q, r)
        used = np.zeros(len(c["P"]), bool)
        used[mem["idx"]] = True
        assert 0.01 < used.mean() < 0.9 and mem["lengths"].max() >= longest
        values = c["values"].copy()
        values[~used] = poison[np.arange((~used).sum()) % 3][:, None]
        for weight in rd.WEIGHTS:
            want = rd.sums(mem, values, weight, r, rd.bandwidth(r))
            assert np.isfinite(want["out"]).all()
            for fallback in ("0", "1"):
                monkeypatch.setenv(FALLBACK, fallback)
                for C in (3, 16):
                    for normalize in (False, True):
                        got = reduce(eng, values, Q, r, weight, C, "ext", normalize)
                        assert np.isfinite(got["out"]).all() and np.isfinite(got["wsum"]).all(), (label, weight, C, fallback)
                        check(got, want, weight, r, len(Q), normalize, fallback == "1")
    c = rd.case("n1025")
    build(eng, c)
    # the skipped self: every point a query, a radius below every distance, every value NaN -- nothing is a neighbour
    r = np.nextafter(rd._nearest(c["P"], c["P"]), np.float32(0))
    assert rd.members(c["P"], None, r, skip_self=True)["lengths"].sum() == 0
    values = np.full_like(c["values"], np.nan)
    for fallback in ("0", "1"):
        monkeypatch.setenv(FALLBACK, fallback)
        for weight in rd.WEIGHTS:
            for normalize in (False, True):
                got = reduce(eng, values, None, r, weight, 16, "own_skip", normalize)
                assert (got["out"] == 0).all() and (got["wsum"] == 0).all() and (got["counts"] == 0).all()
    # a NaN value of a TRUE neighbour propagates
    values = c["values"].copy()
    r = c["radii"]["mid"]
    mem = rd.members(c["P"], Q, r)
    hit = int(mem["idx"][0])
    values[hit, 1] = np.nan
    rows_with = np.array([hit in mem["idx"][mem["offsets"][j]:mem["offsets"][j + 1]] for j in range(len(Q))])
    monkeypatch.setenv(FALLBACK, "0")
    got = reduce(eng, values, Q, r, "gauss", 3)
    assert np.array_equal(np.isnan(got["out"][:, 1]), rows_with) and np.isfinite(got["out"][:, [0, 2]]).all()


@pytest.mark.parametrize("name", ("n17", "n1025", "duplicates", "nan", "ids", "batched"))
def test_counts_are_radius_query_row_lengths(eng, name):
    c = rd.case(name)
    build(eng, c)
    for label, r in c["radii"].items():
        rows = eng.radius_query(c["Q"], float(r), sort=False, want_dist=False)
        lengths = np.diff(rows["offsets"].cpu().numpy())
        got = reduce(eng, c["values"], c["Q"], r, "one", 0)
        assert np.array_equal(got["counts"], lengths) and got["info"]["total"] == rows["count_info"]["total"]
        assert np.array_equal(got["wsum"], lengths.astype(np.float32))


def test_outputs_singly_and_no_queries(eng):
    """The raw call: each output asked for alone, nothing written outside it; m = 0 succeeds with a zeroed info."""
    import torch

    from owlraytracing_amd import _reduce_lib

    lib = _reduce_lib.load()
    c = rd.case("n1025")
    build(eng, c)
    r, C, m, guard = c["radii"]["mid"], 5, len(c["Q"]), 256
    want = want_for("n1025", "mid", "ext", "gauss")
    dev = eng.device
    Q = torch.from_numpy(np.array(c["Q"])).to(dev)
    values = torch.from_numpy(np.ascontiguousarray(c["values"][:, :C])).to(dev)

    def call(counts, wsum, out, channels=C, queries=Q, rows=m, flags=0):
        o, info = _reduce_lib.RadiusReduceOptions(), _reduce_lib.RadiusReduceInfo()
        o.m, o.radius, o.bandwidth, o.weight, o.channels, o.flags = rows, float(r), float(rd.bandwidth(r)), _reduce_lib.W_GAUSS, channels, flags
        o.d_queries, o.d_values = queries.data_ptr(), values.data_ptr() if channels else None
        o.d_counts = None if counts is None else counts[guard:].data_ptr()
        o.d_wsum = None if wsum is None else wsum[guard:].data_ptr()
        o.d_out = None if out is None else out[guard * C:].data_ptr()
        info.total, info.walk_ms = -5, -5.0
        with torch.cuda.device(dev):
            rc = lib.tknnRadiusReduce(eng._h, ctypes.byref(o), ctypes.byref(info), eng._stream())
        assert rc == 0, lib.tknnLastError()
        return info

    def fresh():
        return (torch.full((m + 2 * guard,), -7, dtype=torch.int32, device=dev), torch.full((m + 2 * guard,), -7.0, dtype=torch.float32, device=dev),
                torch.full(((m + 2 * guard) * C,), -7.0, dtype=torch.float32, device=dev))

    def inner(t, per=1):
        return t[guard * per:(guard + m) * per].cpu().numpy()

    def guards_kept(t, per=1):
        return bool((t[:guard * per] == -7).all()) and bool((t[(guard + m) * per:] == -7).all())

    counts, wsum, out = fresh()
    assert call(counts, None, None, channels=0).total == want["counts"].sum()
    rd.compare({"counts": inner(counts)}, want, "gauss", r, rd.bandwidth(r))
    assert guards_kept(counts) and (wsum == -7).all() and (out == -7).all()
    counts, wsum, out = fresh()
    call(None, wsum, None, channels=0)
    rd.compare({"wsum": inner(wsum)}, want, "gauss", r, rd.bandwidth(r))
    assert guards_kept(wsum) and (counts == -7).all() and (out == -7).all()
    counts, wsum, out = fresh()
    call(None, None, out)
    rd.compare({"out": inner(out, C).reshape(m, C)}, want, "gauss", r, rd.bandwidth(r), channels=C)
    assert guards_kept(out, C) and (counts == -7).all() and (wsum == -7).all()
    counts, wsum, out = fresh()
    call(counts, wsum, out, flags=_reduce_lib.REDUCE_NORMALIZE)
    rd.compare({"counts": inner(counts), "wsum": inner(wsum), "out": inner(out, C).reshape(m, C)}, want, "gauss", r, rd.bandwidth(r), normalize=True, channels=C)
    assert guards_kept(counts) and guards_kept(wsum) and guards_kept(out, C)
    # no queries
    counts, wsum, out = fresh()
    info = call(counts, wsum, out, rows=0)
    assert info.total == 0 and info.walk_ms == 0 and info.max_row == 0
    assert (counts == -7).all() and (wsum == -7).all() and (out == -7).all()
    got = eng.radius_reduce(r, queries=np.zeros((0, 3), np.float32), values=c["values"][:, :2])
    assert tuple(got["out"].shape) == (0, 2) and tuple(got["counts"].shape) == (0,) and got["info"]["total"] == 0


def test_knn_and_the_tree_are_left_alone(eng):
    c = rd.case("n1025")
    build(eng, c)
    before = eng.knn(k=8)
    tree_before = eng.export_tree_ex()
    r = c["radii"]["mid"]
    check(reduce(eng, c["values"], c["Q"], r, "gauss", 16), want_for("n1025", "mid", "ext", "gauss"), "gauss", r, len(c["Q"]))
    check(reduce(eng, c["values"], None, r, "one", 4, "own"), want_for("n1025", "mid", "own", "one"), "one", r, len(c["P"]))
    after = eng.knn(k=8)
    assert np.array_equal(before["idx"].cpu().numpy(), after["idx"].cpu().numpy())
    assert np.array_equal(before["dist"].cpu().numpy().view(np.int32), after["dist"].cpu().numpy().view(np.int32))
    tree_after = eng.export_tree_ex()
    for name, a in tree_before.items():
        assert np.array_equal(np.asarray(a), np.asarray(tree_after[name])), name


def test_front_end_and_one_shot(eng):
    import torch

    import owlraytracing_amd
    from owlraytracing_amd.trueknn import radius_reduce as one_shot

    c = rd.case("ids")
    build(eng, c)
    r = c["radii"]["mid"]
    h = rd.bandwidth(r)
    want = want_for("ids", "mid", "ext", "gauss")
    for helper in (one_shot, owlraytracing_amd.radius_reduce):
        got = helper(c["P"], c["Q"], r, ids=c["ids"], values=c["values"][:, :3], weight="gauss", bandwidth=h)
        rd.compare(got, want, "gauss", r, h, channels=3)
    # tensors on the device; (n,) values give (m,) sums; a mean-shift step: the coordinates as values, normalised
    got = eng.radius_reduce(r, queries=torch.from_numpy(np.array(c["Q"])).to(eng.device), values=torch.from_numpy(c["values"][:, 0].copy()).to(eng.device),
                            weight="gauss", bandwidth=h)
    assert tuple(got["out"].shape) == (len(c["Q"]),)
    rd.compare({"out": got["out"].cpu().numpy().reshape(-1, 1), "counts": got["counts"].cpu().numpy()}, want, "gauss", r, h, channels=1)
    bare = eng.radius_reduce(r, queries=c["Q"], want_wsum=False)
    assert "wsum" not in bare and bare["out"] is None and np.array_equal(bare["counts"].cpu().numpy(), want["counts"])
    mem = rd.rows_of("ids", "mid", "own")
    shift = rd.sums(mem, c["P"], "gauss", r, h)
    got = eng.radius_reduce(r, values=c["P"], weight="gauss", bandwidth=h, normalize=True)
    rd.compare({k: v.cpu().numpy() for k, v in got.items() if k != "info"}, shift, "gauss", r, h, normalize=True, channels=3)
    for bad in (dict(weight="box"), dict(weight="gauss"), dict(values=c["values"][:-1]), dict(values=np.zeros((len(c["P"]), 17), np.float32))):
        with pytest.raises(ValueError):
            eng.radius_reduce(r, queries=c["Q"], **bad)
