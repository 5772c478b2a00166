"""TrueKNN.query (tknnQuery: neighbours of points that are not in the tree) against tests/query_spec.py on a GPU: every
row of every set, bit for bit -- indices, distances as int32 views, intersections, levels.

| set        | P                               | Q                                                                  |
|------------|---------------------------------|--------------------------------------------------------------------|
| uniform    | 20 000 uniform 3-D              | 5 000 in the same cube; 500 in a cube twice as wide (many levels)  |
| copies     | the uniform P                   | 2 000 rows of P itself, shuffled: neighbour 0 is at distance 0     |
| lattice    | a lattice with holes            | nodes, cell centres, edge midpoints: ties across rounds            |
| duplicates | a set with repeated points      | uniform + the repeated points                                      |
| planar     | 2-D set (z = 0)                 | 2-D queries and queries off the plane                              |
| clustered  | 64-component mixture            | uniform over the bounding box: boxes grow over whole clusters      |
| tiny       | n = k = 5                       | 3 queries: n >= k is enough                                        |
| scale_*    | (uniform + 1e3) * 1e-6 and 1e+6 | same transform                                                     |
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_rows_equal

sys.path.insert(0, os.path.join(ROOT, "tests"))
import query_spec as qs  # noqa: E402

pytestmark = pytest.mark.gpu

_cache = {}


def _set(name):
    if name not in _cache:
        P, Q, r0 = qs.make_set(name)
        _cache[name] = (P, Q, r0, qs.query_rows(P, Q, qs.ks_for(name), r0))
    return _cache[name]


def _engine(P, ids=None):
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    eng.build(P, ids=ids)
    return eng


def _check(r, spec, what):
    idx, dist = r["idx"].cpu().numpy(), r["dist"].cpu().numpy()
    fin = spec["levels"] >= 0
    assert np.array_equal(r["levels"].cpu().numpy(), spec["levels"]), "%s: levels differ" % what
    assert np.array_equal(r["intersections"].cpu().numpy()[fin], spec["intersections"][fin]), "%s: intersections differ" % what
    assert_rows_equal(idx[fin], dist[fin], spec["idx"][fin], spec["dist"][fin])
    info = r["info"]
    for name in ("rounds", "total_intersections", "total_active_rounds", "unfinished"):
        assert info[name] == spec[name], "%s: info[%s] = %s, the spec says %s" % (what, name, info[name], spec[name])
    assert np.float32(info["final_radius"]) == np.float32(spec["final_radius"]), what


@pytest.mark.parametrize("name", qs.SET_NAMES)
def test_rows_equal_the_spec(name):
    from owlraytracing_amd import _lib

    P, Q, r0, spec = _set(name)
    eng = _engine(P)
    for k in qs.ks_for(name):
        r = eng.query(Q, k, r0, want_levels=True)
        assert r["info"]["kernel_used"] == _lib.KERNEL_QUERY
        _check(r, spec[k], "%s k=%d" % (name, k))
    eng.close()


@pytest.mark.parametrize("name", qs.SET_NAMES)
def test_exact_rows_equal_brute_force(name):
    P, Q, r0, spec = _set(name)
    eng = _engine(P)
    differ = 0
    for k in qs.ks_for(name, (1, 10, 64)):
        want_idx, want_dist = qs.exact_rows(P, Q, k)
        r = eng.query(Q, k, r0, exact=True, want_levels=True)
        idx, dist = r["idx"].cpu().numpy(), r["dist"].cpu().numpy()
        assert np.array_equal(r["levels"].cpu().numpy(), spec[k]["levels"]) and (spec[k]["levels"] >= 0).all()
        assert np.array_equal(r["intersections"].cpu().numpy(), spec[k]["intersections"])
        assert np.array_equal(dist.view(np.int32), want_dist.view(np.int32)), "%s k=%d: exact distances differ" % (name, k)
        assert np.array_equal(idx, want_idx), "%s k=%d: %d exact rows differ in their indices" % (name, k, (idx != want_idx).any(axis=1).sum())
        plain = spec[k]
        differ += int(((plain["idx"] != want_idx).any(axis=1) | (plain["dist"].view(np.int32) != want_dist.view(np.int32)).any(axis=1)).sum())
    if name == "lattice":  # (at k = 1 the nearest candidate of a finished box is the nearest point: the rows that differ are at k = 10 and 64)
        assert differ > 0, "lattice: plain and exact rows are the same everywhere, so the flag was not tested"
    eng.close()


def test_id_built_tree_reports_ids():
    P, Q, r0 = qs.make_set("lattice")
    rng = np.random.default_rng(41)
    ids = ((1 << 30) + rng.permutation(len(P))).astype(np.int32)
    spec = qs.query_rows(P, Q, (3, 10, 16), r0, ids=ids)
    eng = _engine(P, ids=ids)
    for k in (3, 10, 16):
        _check(eng.query(Q, k, r0, want_levels=True), spec[k], "ids k=%d" % k)
        want_idx, want_dist = qs.exact_rows(P, Q, k, ids=ids)
        r = eng.query(Q, k, r0, exact=True)
        assert np.array_equal(r["idx"].cpu().numpy(), want_idx) and np.array_equal(r["dist"].cpu().numpy().view(np.int32), want_dist.view(np.int32))
    eng.close()


def test_query_order_does_not_matter():
    P, Q, r0, spec = _set("uniform")
    perm = np.random.default_rng(42).permutation(len(Q))
    eng = _engine(P)
    a = eng.query(Q, 10, r0, want_levels=True)
    b = eng.query(np.ascontiguousarray(Q[perm]), 10, r0, want_levels=True)
    for name in ("idx", "dist", "intersections", "levels"):
        x, y = a[name].cpu().numpy(), b[name].cpu().numpy()
        assert np.array_equal(x[perm].view(np.int32) if name == "dist" else x[perm], y.view(np.int32) if name == "dist" else y), name
    eng.close()


def test_query_of_the_set_itself_is_self_plus_solve():
    """On a set without repeated points query(P, k + 1) is [self at distance 0] + solve(k), same levels and the same
    intersections (the solve counts the query's own box, the query call the coincident point of P); and a solve gives the
    same before and after a query: the tree and the per-slot state are not disturbed."""
    P, _, r0, _ = _set("uniform")
    k = 10
    eng = _engine(P)
    before = eng.solve(k, r0, want_levels=True)
    q = eng.query(P, k + 1, r0, want_levels=True)
    after = eng.solve(k, r0, want_levels=True)
    for name in ("idx", "dist", "intersections", "levels"):
        assert np.array_equal(before[name].cpu().numpy(), after[name].cpu().numpy()), "solve changed by a query: %s" % name
    qi, qd = q["idx"].cpu().numpy(), q["dist"].cpu().numpy()
    assert np.array_equal(qi[:, 0], np.arange(len(P))) and (qd[:, 0] == 0).all()
    assert np.array_equal(q["levels"].cpu().numpy(), before["levels"].cpu().numpy())
    assert np.array_equal(q["intersections"].cpu().numpy(), before["intersections"].cpu().numpy())
    assert_rows_equal(qi[:, 1:], qd[:, 1:], before["idx"].cpu().numpy(), before["dist"].cpu().numpy())
    eng.close()


def test_unfinished_queries():
    import torch

    from owlraytracing_amd import _lib

    P, Q, r0, _ = _set("uniform")
    wide = np.ascontiguousarray(Q[-qs.N_WIDE:])
    k = 10
    eng = _engine(P)
    for max_rounds in (2, 4):  # 2: none of the wide queries finishes; 4: both kinds of rows in one call
        spec = qs.query_rows(P, wide, (k,), r0, max_rounds=max_rounds)[k]
        assert spec["unfinished"] > 0 and (max_rounds == 2 or spec["unfinished"] < len(wide)), "%d unfinished" % spec["unfinished"]
        out = {"idx": torch.full((len(wide), k), -7, dtype=torch.int32, device=eng.device),
               "dist": torch.full((len(wide), k), -7.0, dtype=torch.float32, device=eng.device),
               "intersections": torch.full((len(wide),), -7, dtype=torch.int64, device=eng.device)}
        r = eng.query(wide, k, r0, max_rounds=max_rounds, allow_unfinished=True, out=out)
        left = spec["levels"] < 0
        assert (r["idx"].cpu().numpy()[left] == -7).all() and (r["dist"].cpu().numpy()[left] == -7).all()
        assert (r["intersections"].cpu().numpy()[left] == -7).all()
        _check(r, spec, "max_rounds=%d" % max_rounds)
    with pytest.raises(_lib.TknnError) as e:
        eng.query(wide, k, r0, max_rounds=2)
    assert e.value.code == -4
    eng.close()


def test_nan_query_and_no_queries():
    P, Q, r0, _ = _set("lattice")
    Qn = Q[:8].copy()
    Qn[3, 1] = np.nan
    spec = qs.query_rows(P, Qn, (4,), r0, max_rounds=6)[4]
    assert spec["levels"][3] == -1 and spec["unfinished"] == 1
    eng = _engine(P)
    _check(eng.query(Qn, 4, r0, max_rounds=6, allow_unfinished=True), spec, "NaN query")
    r = eng.query(np.zeros((0, 3), np.float32), 4, r0, want_levels=True, allow_unfinished=True)
    assert tuple(r["idx"].shape) == (0, 4) and r["info"]["rounds"] == 0 and r["info"]["solve_ms"] == 0 and r["info"]["unfinished"] == 0
    eng.close()


def test_error_codes_in_order():
    import torch

    from owlraytracing_amd import _lib
    from owlraytracing_amd.trueknn import TrueKNN

    lib = _lib.load()
    P, Q, r0 = qs.make_set("tiny")
    eng = TrueKNN(device=0)
    dev = eng.device
    q = torch.from_numpy(Q).to(dev)
    levels = torch.empty(len(Q), dtype=torch.int32, device=dev)
    info = _lib.SolveInfo()

    def call(handle=None, options=True, **kw):
        o = _lib.QueryOptions()
        o.d_queries, o.m, o.k, o.start_radius, o.max_rounds = q.data_ptr(), len(Q), 3, r0, 64
        for name, v in kw.items():
            setattr(o, name, v)
        return lib.tknnQuery(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info), None)

    ARG, STATE, ROUNDS, UNSUPPORTED = -1, -3, -4, -5
    assert call(handle=ctypes.c_void_p()) == ARG and call(options=False) == ARG and call(d_queries=None) == ARG
    assert call() == STATE and call(k=0) == STATE  # not built: before any look at the values
    eng.build(P)
    assert call() == 0
    assert call(k=0) == ARG and call(k=6) == ARG and call(k=100) == ARG  # k > n comes before k > 64
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(start_radius=bad) == ARG
    assert call(m=-1) == ARG and call(allow_unfinished=1) == ARG
    assert call(allow_unfinished=1, d_levels=levels.data_ptr()) == 0
    assert call(m=0, d_queries=None) == 0 and info.rounds == 0
    assert call(max_rounds=1, start_radius=1e-6) == ROUNDS
    with pytest.raises(_lib.TknnError) as e:
        eng.solve(3, r0, kernel=_lib.KERNEL_QUERY)
    assert e.value.code == ARG
    eng.close()
    big = _engine(qs.make_set("lattice")[0])
    o = _lib.QueryOptions()
    o.d_queries, o.m, o.k, o.start_radius = q.data_ptr(), len(Q), 65, r0
    assert lib.tknnQuery(big._h, ctypes.byref(o), ctypes.byref(info), None) == UNSUPPORTED
    o.k = 3
    assert lib.tknnQuery(big._h, ctypes.byref(o), ctypes.byref(info), None) == 0
    big.set_halo(P, np.arange(5, dtype=np.int32) + 5000)
    assert lib.tknnQuery(big._h, ctypes.byref(o), ctypes.byref(info), None) == UNSUPPORTED
    o.k = 65  # k > 64 is reported before the halo
    assert lib.tknnQuery(big._h, ctypes.byref(o), ctypes.byref(info), None) == UNSUPPORTED and b"k out of range" in lib.tknnLastError()
    big.set_halo(None)
    o.k = 3
    assert lib.tknnQuery(big._h, ctypes.byref(o), ctypes.byref(info), None) == 0
    big.close()


def test_python_argument_checks():
    import torch

    P, Q, r0 = qs.make_set("tiny")
    eng = _engine(P)
    q = torch.from_numpy(Q).to(eng.device)
    for bad in (q.double(), q[:, :2], q.cpu(), q.t().contiguous().t(), Q.astype(np.float32).reshape(-1)):
        with pytest.raises(ValueError):
            eng.query(bad, 3, r0)
    for name, t in (("idx", torch.empty((3, 3), dtype=torch.int64, device=eng.device)), ("dist", torch.empty((3, 4), dtype=torch.float32, device=eng.device)),
                    ("intersections", torch.empty((3,), dtype=torch.int64)), ("idx", torch.empty((3, 6), dtype=torch.int32, device=eng.device)[:, ::2]),
                    ("fb", torch.empty((3,), dtype=torch.uint8, device=eng.device))):
        with pytest.raises(ValueError):
            eng.query(q, 3, r0, out={name: t})
    assert tuple(eng.query(q, 3, r0)["idx"].shape) == (3, 3)
    eng.close()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import query_spec as qs
from owlraytracing_amd.trueknn import TrueKNN
P, Q, r0 = qs.make_set("lattice")
spec = qs.query_rows(P, Q, (10, 33), r0)
eng = TrueKNN(device=0)
eng.build(P)
for k in (10, 33):
    r = eng.query(Q, k, r0, want_levels=True)
    assert r["info"]["tie_rows"] == 0, r["info"]
    for name in ("idx", "intersections", "levels"):
        assert np.array_equal(r[name].cpu().numpy(), spec[k][name]), (k, name)
    assert np.array_equal(r["dist"].cpu().numpy().view(np.int32), spec[k]["dist"].view(np.int32)), k
    want_idx, want_dist = qs.exact_rows(P, Q, k)
    r = eng.query(Q, k, r0, exact=True)
    assert np.array_equal(r["idx"].cpu().numpy(), want_idx) and np.array_equal(r["dist"].cpu().numpy().view(np.int32), want_dist.view(np.int32)), k
print("fallback ok")
"""


def test_forced_fallback_in_a_child_process():
    """TKNN_QUERY_FORCE_FALLBACK=1: the walk leaves every query to the one-query-per-lane kernel, as it does on stack exhaustion."""
    env = dict(os.environ, TKNN_QUERY_FORCE_FALLBACK="1")
    p = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "fallback ok" in p.stdout, p.stdout + p.stderr


def test_cli_prints_the_rows(tmp_path):
    from owlraytracing_amd import datasets

    P, Q, r0 = qs.make_set("lattice")
    Q = Q[:40]
    datasets.write_csv_points(str(tmp_path / "p.csv"), P)
    datasets.write_csv_points(str(tmp_path / "q.csv"), Q)
    P2 = datasets.pad_to_3d(datasets.read_csv_points(str(tmp_path / "p.csv"), len(P), 3))
    Q2 = datasets.pad_to_3d(datasets.read_csv_points(str(tmp_path / "q.csv"), len(Q), 3))
    for extra, (want_idx, want_dist) in (([], (lambda s: (s["idx"], s["dist"]))(qs.query_rows(P2, Q2, (5,), r0)[5])), (["--exact"], qs.exact_rows(P2, Q2, 5))):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "trueknn_cli.py"), str(tmp_path / "p.csv"), str(len(P)), "3", repr(r0), "5",
                            str(tmp_path / "t.txt"), "--queries", str(tmp_path / "q.csv")] + extra, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        rows = [ln for ln in p.stdout.splitlines() if ln[:1].isdigit() and ": " in ln]
        assert len(rows) == len(Q)
        for j, ln in enumerate(rows):
            head, rest = ln.split(": ", 1)
            a, b = rest.split(" | ")
            assert int(head) == j and [int(v) for v in a.split()] == list(want_idx[j])
            assert np.array_equal(np.array([float(v) for v in b.split()], np.float32).view(np.int32), want_dist[j].view(np.int32))
