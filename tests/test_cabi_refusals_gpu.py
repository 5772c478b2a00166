"""What the C-ABI (include/owlknn.h) refuses, and with which code: one table of (call, arguments with exactly one fault,
expected code), driven through ctypes on three engines -- one not built, one built on 10 points, one on 100 -- the smallest
shapes at which every check can still fire (k = 65 is above 10 points and below 100).  Every row is an argument the library
rejects before it launches anything; after every row the engine must still solve its points correctly.

The table holds every refusal of the extern "C" layer (csrc/tknn_api.hip) and, of the engine's own, the halo selection's
npeers range; the engine's other refusals that a call reaches before any kernel is launched -- Engine::solve's and the fill
pass of tknnRadiusQuery whose rows do not fit -- are test_refusals_of_the_engine_behind_an_accepted_call: the C layer has accepted
those calls, so info is zeroed, and two of the messages do not name the function.  No test here depends on another having run.

The order of the checks is part of what is pinned: required pointers, then the engine's state (TKNN_E_STATE before
tknnBuild), then values -- and among the values of tknnQuery and tknnSolveEx the order the precedence rows name."""
import ctypes
import os
import sys

import numpy as np
import pytest

import oracle
from conftest import ROOT, assert_rows_equal
from owlraytracing_amd import _lib, datasets

sys.path.insert(0, os.path.join(ROOT, "tests"))
import cabi_calls as cc  # noqa: E402
from cabi_calls import DEV, E_ARG, E_ROUNDS, E_STATE, E_UNSUPPORTED, OK, TOO_MANY  # noqa: E402

pytestmark = pytest.mark.gpu

NONE, N10, N100 = "not built", "10 points", "100 points"
SIZES = {N10: (10, 3), N100: (100, 5)}  # engine: (points, the k of the solve that follows every row)
R0 = 0.1
INF, NAN = float("inf"), float("nan")
SPARE_BYTES = 4 << 20  # what every DEV address points at: room for any output of a call on 100 points, should a refusal not come
FILL = 0x5A


def _rows():
    rows = []

    def row(fn, engine, code, **faults):
        if (fn, engine, code, faults) not in rows:
            rows.append((fn, engine, code, faults))

    # required pointers: TKNN_E_ARG, built or not
    pointers = [
        ("tknnBuild", dict(d_xyz=None)), ("tknnBuildIds", dict(d_xyz=None)),
        ("tknnSetHalo", dict(d_xyz=None)), ("tknnSetHalo", dict(d_ids=None)),
        ("tknnHaloSelect", dict(d_boxes=None)), ("tknnHaloSelect", dict(d_box_peer=None)),
        ("tknnHaloSelect", dict(d_counts=None)),  # neither counts (count pass) nor rows (write pass)
        ("tknnHaloSelect", dict(d_rows=DEV)),  # rows without offsets
        ("tknnSolveEx", dict(options=None)),
        ("tknnQuery", dict(options=None)), ("tknnQuery", dict(d_queries=None)),
        ("tknnDbscan", dict(d_labels=None)),
        ("tknnDbscanAssign", dict(d_core_label=None)), ("tknnDbscanAssign", dict(d_labels=None)),
        ("tknnDbscanQuery", dict(options=None)), ("tknnDbscanQuery", dict(d_core_label=None)), ("tknnDbscanQuery", dict(d_labels=None)),
        ("tknnDbscanQuery", dict(d_queries=None)),
        ("tknnRadiusQuery", dict(options=None)), ("tknnRadiusQuery", dict(d_offsets=None)), ("tknnRadiusQuery", dict(d_queries=None)),
        ("tknnRadiusKnn", dict(options=None)), ("tknnRadiusKnn", dict(d_idx=None)), ("tknnRadiusKnn", dict(d_queries=None)),
        ("tknnDbscanAuto", dict(d_labels=None)), ("tknnDbscanNoise", dict(d_noise=None)),
        ("tknnExportTreeEx", dict(x=None)),
    ]
    pointers += [("tknnHaloSelectFixed", {name: None}) for name in ("d_boxes", "d_box_peer", "d_caps", "d_offsets", "d_rows", "d_counts")]
    pointers += [("tknnRepairExact", {name: None}) for name in ("d_levels", "d_idx", "d_dist")]
    pointers += [("tknnSegmentMin", {name: None}) for name in ("d_segment", "d_value", "d_out")]
    # ... and the values that are checked with them, before the engine's state
    early = [("tknnSetHalo", dict(m=-1)), ("tknnSetHalo", dict(m=TOO_MANY)), ("tknnHaloSelect", dict(nboxes=-1)),
             ("tknnHaloSelectFixed", dict(nboxes=-1)), ("tknnSegmentMin", dict(n=-1)),
             ("tknnExportTreeEx", dict(which=2)), ("tknnExportTreeEx", dict(which=-1)), ("tknnExportTreeEx", dict(wide_capacity=-1))]
    early += [(fn, dict(n=n)) for fn in ("tknnBuild", "tknnBuildIds") for n in (0, -1, TOO_MANY)]
    for fn, faults in pointers + early:
        for engine in (NONE, N10):
            row(fn, engine, E_ARG, **faults)

    # before tknnBuild: TKNN_E_STATE, with good values and with a bad one
    for fn, bad in (("tknnSetHalo", {}), ("tknnHaloSelect", dict(npeers=0)), ("tknnHaloSelectFixed", dict(npeers=0)),
                    ("tknnSolve", dict(k=0)), ("tknnSolveEx", dict(k=0)), ("tknnSolveEx", dict(start_radius=0.0)), ("tknnSolveEx", dict(phase=7)),
                    ("tknnSolveEx", dict(k=1025)), ("tknnRepairExact", dict(k=0)), ("tknnRepairExact", dict(start_radius=NAN)),
                    ("tknnQuery", dict(k=0)), ("tknnQuery", dict(m=-1)), ("tknnQuery", dict(k=65)), ("tknnQuery", dict(allow_unfinished=1)),
                    ("tknnDbscan", dict(eps=0.0)), ("tknnDbscan", dict(min_pts=0)), ("tknnDbscanAssign", dict(eps=0.0)),
                    ("tknnDbscanQuery", dict(eps=0.0)), ("tknnDbscanQuery", dict(m=-1)),
                    ("tknnRadiusQuery", dict(radius=0.0)), ("tknnRadiusQuery", dict(m=-1)), ("tknnRadiusQuery", dict(capacity=-1)),
                    ("tknnRadiusQuery", dict(d_dist=DEV)), ("tknnRadiusKnn", dict(k=0)), ("tknnRadiusKnn", dict(k=65)), ("tknnRadiusKnn", dict(radius=0.0)),
                    ("tknnDbscanAuto", dict(eps0=0.0)), ("tknnDbscanAuto", dict(max_rounds=0)), ("tknnDbscanNoise", dict(min_pts=0)),
                    ("tknnExportTree", {}), ("tknnExportTreeTables", {}), ("tknnExportTreeEx", dict(which=1))):
        row(fn, NONE, E_STATE)
        if bad:
            row(fn, NONE, E_STATE, **bad)

    # values, on a built engine
    bad_radius = (0.0, -1.0, INF, NAN)
    for fn in ("tknnSolve", "tknnSolveEx"):
        for k in (0, -1, 10):  # (10: the reference never terminates with k >= n)
            row(fn, N10, E_ARG, k=k)
        row(fn, N100, E_ARG, k=100)
        row(fn, N10, E_UNSUPPORTED, k=1025)  # above TKNN_MAX_K: said before "k >= n"
        row(fn, N100, E_UNSUPPORTED, k=1025)
        for r in bad_radius:
            row(fn, N10, E_ARG, start_radius=r)
        for kernel in (-1, 4):
            row(fn, N10, E_ARG, kernel=kernel)
    for phase in (-1, 4):
        row("tknnSolveEx", N10, E_ARG, phase=phase)
    for k in (0, 65):
        row("tknnRepairExact", N100, E_ARG, k=k)
    for r in bad_radius:
        row("tknnRepairExact", N10, E_ARG, start_radius=r)
    for k in (0, -1, 11, 65):  # (65 on 10 points: "n >= k" is said before "k <= 64")
        row("tknnQuery", N10, E_ARG, k=k)
    row("tknnQuery", N100, E_ARG, k=101)
    row("tknnQuery", N100, E_UNSUPPORTED, k=65)
    for r in bad_radius:
        row("tknnQuery", N10, E_ARG, start_radius=r)
    row("tknnQuery", N10, E_ARG, allow_unfinished=1)  # without d_levels
    for fn in ("tknnQuery", "tknnDbscanQuery", "tknnRadiusQuery", "tknnRadiusKnn"):
        for m in (-1, TOO_MANY):
            row(fn, N10, E_ARG, m=m)
    for fn, name in (("tknnDbscan", "eps"), ("tknnDbscanAssign", "eps"), ("tknnDbscanQuery", "eps"), ("tknnDbscanNoise", "eps"),
                     ("tknnDbscanAuto", "eps0"), ("tknnRadiusQuery", "radius"), ("tknnRadiusKnn", "radius")):
        for r in bad_radius:
            row(fn, N10, E_ARG, **{name: r})
    for fn in ("tknnDbscan", "tknnDbscanNoise", "tknnDbscanAuto"):
        for min_pts in (0, -1):
            row(fn, N10, E_ARG, min_pts=min_pts)
    for max_noise in (-0.1, 1.1, NAN):
        row("tknnDbscanAuto", N10, E_ARG, max_noise=max_noise)
    row("tknnDbscanAuto", N10, E_ARG, max_rounds=0)
    row("tknnRadiusQuery", N10, E_ARG, d_dist=DEV)  # without d_idx
    row("tknnRadiusQuery", N10, E_ARG, capacity=-1)
    for k in (0, -1):
        row("tknnRadiusKnn", N10, E_ARG, k=k)
    for engine in (N10, N100):  # (no "n >= k" here: short rows are padded)
        row("tknnRadiusKnn", engine, E_UNSUPPORTED, k=65)
    for fn in ("tknnHaloSelect", "tknnHaloSelectFixed"):
        for npeers in (0, 65):
            row(fn, N10, E_ARG, npeers=npeers)
    row("tknnExportTreeEx", N10, E_STATE, which=1)  # no halo tree is set
    return rows


ROWS = _rows()


def _row_id(r):
    fn, engine, code, faults = r
    return "%s-%s-%s" % (fn, engine.replace(" ", ""), ",".join("%s=%s" % (k, "DEV" if v == DEV else v) for k, v in faults.items()) or "good")


class _Bench:
    """The three engines, the device memory every DEV address names, and the solve each built engine must still answer."""

    def __init__(self):
        import torch
        self.torch = torch
        self.lib = _lib.load()
        self.spare = torch.full((SPARE_BYTES,), FILL, dtype=torch.uint8, device="cuda")
        self.host = ctypes.create_string_buffer(1 << 16)
        self.engines, self.refs, self.out = {}, {}, {}
        for name in (NONE, N10, N100):
            h = ctypes.c_void_p()
            _lib.check(self.lib.tknnCreate(ctypes.byref(h)))
            self.engines[name] = h
        for name, (n, k) in SIZES.items():
            xyz = datasets.uniform3d(n, seed=7 + n)
            pts = torch.from_numpy(xyz).cuda()
            _lib.check(self.lib.tknnBuild(self.engines[name], ctypes.c_void_p(pts.data_ptr()), n, None, None))
            torch.cuda.synchronize()
            self.refs[name] = oracle.trueknn(xyz, k, R0)
            self.out[name] = (torch.empty((n, k), dtype=torch.int32, device="cuda"), torch.empty((n, k), dtype=torch.float32, device="cuda"))

    def call(self, fn, engine, **faults):
        return cc.call(self.lib, fn, self.engines[engine], self.spare.data_ptr(), ctypes.addressof(self.host), **faults)

    def still_works(self, engine):
        if engine == NONE:
            rc, _, _, _ = self.call("tknnSolve", NONE)
            assert rc == E_STATE
            return
        n, k = SIZES[engine]
        idx, dist = self.out[engine]
        idx.fill_(-9)
        dist.fill_(-9.0)
        rc = self.lib.tknnSolve(self.engines[engine], k, R0, 0, 0, ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(dist.data_ptr()), None, None, None, None)
        assert rc == OK, self.lib.tknnLastError()
        self.torch.cuda.synchronize()
        ref = self.refs[engine]
        assert_rows_equal(idx.cpu().numpy(), dist.cpu().numpy(), ref["idx"], ref["dist"])

    def spare_untouched(self):
        return bool((self.spare == FILL).all())

    def close(self):
        for h in self.engines.values():
            self.lib.tknnDestroy(h)


@pytest.fixture(scope="module")
def bench():
    b = _Bench()
    yield b
    b.close()


@pytest.mark.parametrize("r", ROWS, ids=_row_id)
def test_refusal(bench, r):
    fn, engine, code, faults = r
    rc, message, info, _ = bench.call(fn, engine, **faults)
    assert rc == code, (rc, message)
    assert message.startswith(cc.SPEAKS_AS.get(fn, fn)), message
    assert info is None or info == bytes([cc.INFO_FILL]) * len(info), "a refused call wrote its info"
    assert bench.spare_untouched(), "a refused call wrote through a DEV address"
    bench.still_works(engine)


def test_the_table_covers_every_call():
    assert {fn for fn, _, _, _ in ROWS} == set(cc.CALLS)


def test_refusals_of_the_engine_behind_an_accepted_call(bench):
    """What Engine::solve refuses before it launches anything, through tknnSolveEx, and the fill pass of tknnRadiusQuery whose
    d_offsets[m] is above the capacity."""
    torch = bench.torch
    lane, wave = 1, 2
    for engine, code, faults in ((N100, E_UNSUPPORTED, dict(k=65, kernel=lane)), (N100, E_UNSUPPORTED, dict(k=65, kernel=wave)),
                                 (N10, E_UNSUPPORTED, dict(d_start_radii=DEV, kernel=lane)), (N10, E_UNSUPPORTED, dict(phase=1, kernel=lane)),
                                 (N10, E_ARG, dict(phase=3)),  # without d_levels
                                 (N10, E_STATE, dict(phase=1)), (N10, E_STATE, dict(phase=2))):  # no count pass of tknnHaloSelect since the build
        rc, message, info, _ = bench.call("tknnSolveEx", engine, **faults)
        assert rc == code, (faults, rc, message)
        assert message, faults
        assert info == bytes(len(info)), faults  # (the arguments were accepted)
        assert bench.spare_untouched(), faults
        bench.still_works(engine)
    n = SIZES[N10][0]
    queries = torch.from_numpy(datasets.uniform3d(n, seed=7 + n)[:4].copy()).cuda()
    offsets = torch.zeros((5,), dtype=torch.int64, device="cuda")
    args = dict(d_queries=queries.data_ptr(), m=4, radius=10.0, d_offsets=offsets.data_ptr())
    rc, message, _, _ = bench.call("tknnRadiusQuery", N10, **args)
    torch.cuda.synchronize()
    assert rc == OK, message
    assert offsets.tolist() == [0, 10, 20, 30, 40]
    rc, message, _, _ = bench.call("tknnRadiusQuery", N10, d_idx=DEV, d_dist=DEV, capacity=39, **args)
    assert rc == E_ARG and message.startswith("tknnRadiusQuery") and "capacity" in message, (rc, message)
    assert bench.spare_untouched()
    bench.still_works(N10)


def test_query_is_refused_while_a_halo_tree_is_set(bench):
    torch = bench.torch
    halo = torch.from_numpy(datasets.uniform3d(4, seed=3) + np.float32(2.0)).cuda()
    ids = torch.arange(1000, 1004, dtype=torch.int32, device="cuda")
    rc, message, _, _ = bench.call("tknnSetHalo", N100, d_xyz=halo.data_ptr(), d_ids=ids.data_ptr(), m=4)
    torch.cuda.synchronize()
    assert rc == OK, message
    try:
        rc, message, info, _ = bench.call("tknnQuery", N100)
        assert rc == E_UNSUPPORTED and message.startswith("tknnQuery"), (rc, message)
        assert "tiles" in message
        assert info == bytes([cc.INFO_FILL]) * len(info)
        rc, message, _, _ = bench.call("tknnSolveEx", N100, d_start_radii=DEV)  # (the engine's: the halo is exchanged for one radius)
        assert rc == E_UNSUPPORTED and message.startswith("tknnSolve"), (rc, message)
        assert bench.spare_untouched()
    finally:
        rc, message, _, _ = bench.call("tknnSetHalo", N100, d_xyz=None, d_ids=None, m=0)  # (m = 0 is accepted: it clears the halo)
        assert rc == OK, message
    bench.still_works(N100)


def test_dbscan_auto_out_of_rounds_says_so_in_its_own_name(bench):
    """eps0 so small that every point is noise and one doubling changes nothing: TKNN_E_ROUNDS, not a clustering."""
    try:
        rc, message, _, _ = bench.call("tknnDbscanAuto", N10, eps0=1e-30, min_pts=5, max_noise=0.0, max_rounds=1,
                                       d_labels=bench.spare.data_ptr(), d_core=bench.spare.data_ptr() + SPARE_BYTES // 2)
        bench.torch.cuda.synchronize()
    finally:
        bench.spare.fill_(FILL)  # (the call wrote labels and core flags)
    assert rc == E_ROUNDS, (rc, message)
    assert message.startswith("tknnDbscanAuto") and "max_rounds" in message
    bench.still_works(N10)


@pytest.mark.parametrize("fn", ["tknnQuery", "tknnDbscanQuery", "tknnRadiusQuery", "tknnRadiusKnn"])
def test_no_queries_is_a_call_that_does_nothing(bench, fn):
    """m = 0 (d_queries NULL) is accepted by the four query calls: info comes back zeroed and no output is touched."""
    bench.spare.fill_(FILL)
    faults = dict(m=0, d_queries=None)
    if fn == "tknnRadiusQuery":  # the fill pass: the count pass writes d_offsets[0] (below)
        faults.update(d_idx=DEV, d_dist=DEV, capacity=16)
    rc, message, info, _ = bench.call(fn, N10, **faults)
    bench.torch.cuda.synchronize()
    assert rc == OK, message
    assert info == bytes(len(info))
    assert bench.spare_untouched()
    bench.still_works(N10)


def test_radius_count_pass_without_queries_writes_the_one_offset(bench):
    torch = bench.torch
    offsets = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    bench.spare.fill_(FILL)
    rc, message, info, _ = bench.call("tknnRadiusQuery", N10, m=0, d_queries=None, d_offsets=offsets.data_ptr())
    assert rc == OK, message
    assert info == bytes(len(info))
    assert offsets.tolist() == [0, 77]  # (the call itself waits for the write)
    assert bench.spare_untouched()
    bench.still_works(N10)


def test_an_engine_refused_before_its_build_is_left_usable(bench):
    """An engine of its own takes every row of the table for the engine that is not built, then a build and a solve."""
    n, k = SIZES[N10]
    fresh = ctypes.c_void_p()
    _lib.check(bench.lib.tknnCreate(ctypes.byref(fresh)))
    try:
        for fn, engine, code, faults in ROWS:
            if engine == NONE:
                rc, message, _, _ = cc.call(bench.lib, fn, fresh, bench.spare.data_ptr(), ctypes.addressof(bench.host), **faults)
                assert rc == code, (fn, faults, rc, message)
        pts = bench.torch.from_numpy(datasets.uniform3d(n, seed=7 + n)).cuda()
        _lib.check(bench.lib.tknnBuild(fresh, ctypes.c_void_p(pts.data_ptr()), n, None, None))
        idx, dist = bench.out[N10]
        idx.fill_(-9)
        rc = bench.lib.tknnSolve(fresh, k, R0, 0, 0, ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(dist.data_ptr()), None, None, None, None)
        assert rc == OK, bench.lib.tknnLastError()
        bench.torch.cuda.synchronize()
        assert_rows_equal(idx.cpu().numpy(), dist.cpu().numpy(), bench.refs[N10]["idx"], bench.refs[N10]["dist"])
        assert bench.spare_untouched()
    finally:
        bench.lib.tknnDestroy(fresh)
