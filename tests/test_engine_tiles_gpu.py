"""The engine's tile surface in-process, against the replay: trees built with caller ids (tknnBuildIds), a halo tree
(tknnSetHalo), the boundary marks of tknnHaloSelect and the phase / allow_unfinished / d_levels / d_start_radii options of
tknnSolveEx -- on point sets with exact fp32 distance ties, where the tie pass decides rows.

Expected values: rows from oracle.trueknn on the global set G (ids = positions in G: the replay's tie order by index is the
order by id), per-query levels from oracle.trueknn_numpy, per-query start radii from oracle.trueknn_per_query.  The sets and
layouts are tests/tile_sets.py's; tests/test_tile_expectations.py checks these expectations on the CPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle
import tile_sets
from oracle.trueknn_numpy import trueknn_numpy
from owlraytracing_amd import _lib

from conftest import ROOT, assert_rows_equal

pytestmark = pytest.mark.gpu

KERNELS = {"lane": _lib.KERNEL_LANE, "wave": _lib.KERNEL_WAVE, "team": _lib.KERNEL_TEAM, "auto": _lib.KERNEL_AUTO}
K_ALL = [2, 3, 5, 16, 17, 33, 48, 64, 65, 100]


def _kernels(k):
    # (k > 64: the team walk with the lists in memory, asked for by name or through TKNN_KERNEL_AUTO)
    return ("lane", "wave", "team") if k <= 64 else ("team", "auto")


def _sets(k):
    # the cross-round set is made for r0 = 1 and small k (k = 3: its rows that need the level key tie with no candidate
    # left out, so the tie pass looks at the written row first); the others carry ties at every k
    return (("cross",) if k <= 5 else ()) + ("lattice", "quantised", "duplicates")


_REPLAYS = {}


def _replay(name, k):
    """(G, r0, oracle.trueknn(G, k, r0)), computed once per set and k."""
    if (name, k) not in _REPLAYS:
        xyz, r0 = tile_sets.tie_set(name)
        _REPLAYS[(name, k)] = (xyz, r0, oracle.trueknn(xyz, k, r0))
    return _REPLAYS[(name, k)]


@pytest.fixture(scope="module")
def engines():
    """One engine per (set, layout, id offset), built once and re-solved by every test that uses it."""
    from owlraytracing_amd.trueknn import TrueKNN
    made = {}

    def get(name, layout, ids_offset=0):
        key = (name, layout, ids_offset)
        if key not in made:
            xyz, _ = tile_sets.tie_set(name)
            eng = TrueKNN()
            if layout == "relabel":
                perm = tile_sets.relabel(len(xyz))
                eng.build(xyz[perm], (perm.astype(np.int64) + ids_offset).astype(np.int32))
                eng.layout = perm
            else:
                own, rest = tile_sets.split(xyz)
                eng.build(xyz[own], own)
                eng.layout = (own, rest)
            made[key] = eng
        return made[key]

    yield get
    for eng in made.values():
        eng.close()


def _np(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def _check_rows(r, ref, rows, what, ids_offset=0):
    """Rows of a solve against rows `rows` of a replay: intersection counts, distances bit for bit, ids in order."""
    assert np.array_equal(_np(r["intersections"]), ref["intersections"][rows]), what + ": intersection counts differ"
    try:
        assert_rows_equal(_np(r["idx"]).astype(np.int64) - ids_offset, _np(r["dist"]), ref["idx"][rows], ref["dist"][rows])
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e))


def _has_ties(ref, rows=slice(None)):
    d = ref["dist"][rows]
    return bool((d[:, 1:] == d[:, :-1]).any())


def _check_ties(r, ref, k, what):
    """The set must still carry ties (else the test passes vacuously), and the tie pass must have done every row."""
    assert _has_ties(ref), what + ": the replay's rows hold no exact-distance ties"
    assert r["info"]["tie_rows_left"] == 0, what
    if k <= 64:
        assert r["info"]["tie_rows"] > 0, what
    else:
        assert r["info"]["tie_rows"] == 0, what  # (k > 64: three-word keys, the rows are final as listed)


@pytest.mark.parametrize("k,kernel", [(k, kern) for k in K_ALL for kern in _kernels(k)])
def test_relabelled_tree_without_halo(engines, monkeypatch, k, kernel):
    """(a) local row i holds G[perm[i]] with id perm[i]: every id is below n and none is its row.  The tie pass orders
    tied neighbours by the level at which each became a candidate; its look at the written row must not turn an id into
    a point through the table of rows (that is some other point).  Compact outputs, and the frameBuffer alone (the look
    reads the records), with the look allowed and switched off."""
    for name in _sets(k):
        xyz, r0, ref = _replay(name, k)
        eng = engines(name, "relabel")
        perm = eng.layout
        n = len(xyz)
        want_fb = ref["fb"].reshape(n, k)[perm]
        for look in ("1", "0"):
            monkeypatch.setenv("TKNN_TIE_LOOK", look)
            what = "%s k=%d %s look=%s" % (name, k, kernel, look)
            r = eng.solve(k, r0, kernel=KERNELS[kernel])
            _check_rows(r, ref, perm, what)
            _check_ties(r, ref, k, what)
            fb = _np(eng.solve(k, r0, kernel=KERNELS[kernel], fb_only=True)["fb"]).view(oracle.NEIGH_DTYPE).reshape(n, k)
            for field in ("ind", "dist", "numNeighbors", "intersections"):
                assert np.array_equal(fb[field], want_fb[field]), (what, "fb_only", field)


@pytest.mark.parametrize("offset", [2 ** 30, 2 ** 31 - 4001], ids=["2^30", "top"])
@pytest.mark.parametrize("k,kernel", [(2, "lane"), (2, "wave"), (3, "team"), (5, "team"), (16, "wave"), (33, "team"), (64, "lane"),
                                      (65, "team"), (100, "auto")])
def test_large_ids(engines, k, kernel, offset):
    """(b) ids = perm + offset, every one at or above n.  With offset 2^31 - 4001 the largest id of the 4 000-point sets
    is 2^31 - 2: ids must pass the kernels' 32-bit key words and sort words unchanged."""
    top = 0
    for name in _sets(k):
        xyz, r0, ref = _replay(name, k)
        eng = engines(name, "relabel", offset)
        what = "%s k=%d %s ids+%d" % (name, k, kernel, offset)
        r = eng.solve(k, r0, kernel=KERNELS[kernel])
        _check_rows(r, ref, eng.layout, what, ids_offset=offset)
        _check_ties(r, ref, k, what)
        top = max(top, int(_np(r["idx"]).max()))
    assert top == (2 ** 31 - 2 if offset == 2 ** 31 - 4001 else 2 ** 30 + 3999)


@pytest.mark.parametrize("k,kernel", [(k, kern) for k in (2, 3, 5, 17, 48, 65, 100) for kern in _kernels(k)])
def test_tile_with_halo(engines, k, kernel):
    """(c) the tile on one side of a plane in shuffled order (ids = positions in G, not monotone), the complement as the
    halo tree, phase 0: every row is the global replay's."""
    _tile_with_halo(engines, k, kernel)


def _tile_with_halo(engines, k, kernel):
    for name in _sets(k):
        xyz, r0, ref = _replay(name, k)
        eng = engines(name, "split")
        own, rest = eng.layout
        eng.set_halo(xyz[rest], rest)
        try:
            r = eng.solve(k, r0, kernel=KERNELS[kernel])
        finally:
            eng.set_halo(None, None)
        what = "%s k=%d %s halo" % (name, k, kernel)
        _check_rows(r, ref, own, what)
        _check_ties(r, ref, k, what)


@pytest.mark.parametrize("k", [48, 64])
def test_tile_with_halo_through_the_team_walk_alone(engines, monkeypatch, k):
    """(c) once more with TKNN_TEAM_WALK_ALL=1: no packet kernel, every query of the tile walks both trees from level 0
    (the engine picks the walk's halo instantiation from the halo tree being set), four list registers per lane -- k = 64
    fills the list, k = 48 does not."""
    monkeypatch.setenv("TKNN_TEAM_WALK_ALL", "1")
    _tile_with_halo(engines, k, "team")


_TAIL_KS = (5, 17, 33, 48)  # one, two and three list registers per lane (k = 33: the list not full, k = 48: full)
_TAIL_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import tile_sets
from owlraytracing_amd import _lib
from owlraytracing_amd.trueknn import TrueKNN
xyz, r0 = tile_sets.clustered()
own, rest = tile_sets.split(xyz)
eng = TrueKNN()
eng.build(xyz[own], own)
eng.set_halo(xyz[rest], rest)
out = {}
for k in %r:
    print("solve k=%%d" %% k, file=sys.stderr, flush=True)
    r = eng.solve(k, r0, kernel=_lib.KERNEL_TEAM)
    for name in ("idx", "dist", "intersections"):
        out["%%s_%%d" %% (name, k)] = r[name].cpu().numpy()
    out["ties_%%d" %% k] = np.int64([r["info"]["tie_rows"], r["info"]["tie_rows_left"]])
eng.close()
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def walk_tail(tmp_path_factory):
    """The clustered set split by a plane, tile plus halo, solved in ONE child process with TKNN_TEAM_TAIL=walk and
    TKNN_VERBOSE=1 for every k of _TAIL_KS: (the child's stderr per k, its rows)."""
    path = str(tmp_path_factory.mktemp("walk_tail") / "rows.npz")
    env = dict(os.environ, TKNN_TEAM_TAIL="walk", TKNN_VERBOSE="1")
    p = subprocess.run([sys.executable, "-c", _TAIL_CHILD % (ROOT, os.path.join(ROOT, "tests"), _TAIL_KS), path], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    said = {int(part.split(None, 1)[0]): part for part in p.stderr.split("solve k=")[1:]}
    return said, np.load(path)


@pytest.mark.parametrize("k", _TAIL_KS)
def test_tile_with_halo_handed_over_to_the_team_walk(walk_tail, k):
    """(c) with a tail: the clustered set at a start radius far too large for its cores, so that the packet kernel hands
    its queries over, and the team walk (TKNN_TEAM_TAIL=walk; one, two and three list registers per lane) finishes them over both
    trees.  The engine says so (TKNN_VERBOSE), else the case would pass without the walk."""
    said, rows = walk_tail
    m = re.search(r"\[team\] (\d+) of \d+ queries handed over .* team walk ", said[k])
    assert m and int(m.group(1)) > 0, said[k]
    xyz, r0 = tile_sets.clustered()
    own, rest = tile_sets.split(xyz)
    assert len(own) > 0 and len(rest) > 0
    ref = oracle.trueknn(xyz, k, r0)
    assert ref["rounds"] >= 3
    r = {name: rows["%s_%d" % (name, k)] for name in ("idx", "dist", "intersections")}
    r["info"] = {"tie_rows": int(rows["ties_%d" % k][0]), "tie_rows_left": int(rows["ties_%d" % k][1])}
    what = "clustered k=%d team walk tail, halo" % k
    _check_rows(r, ref, own, what)
    _check_ties(r, ref, k, what)


def _sentinel(dev, n, k):
    """Outputs of a solve prefilled with 0xA5 bytes."""
    import torch

    def fill(nbytes, dtype, shape):
        return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev).view(dtype).view(shape)
    return {"idx": fill(n * k * 4, torch.int32, (n, k)), "dist": fill(n * k * 4, torch.float32, (n, k)),
            "intersections": fill(n * 8, torch.int64, (n,)), "levels": fill(n * 4, torch.int32, (n,))}


def _host(out):
    return {name: _np(t).copy() for name, t in out.items() if name != "info"}


_LEVELS = {}


@pytest.mark.parametrize("name,k", [("cross", 2), ("lattice", 5), ("lattice", 16), ("lattice", 33), ("lattice", 64),
                                    ("lattice", 65), ("lattice", 100)])
def test_phases_one_two_three(engines, name, k):
    """(d) the sharded driver's phases, in one thread.  Halo radius = r0 doubled `cap` times; the peer box = the
    complement's bounding box widened by it, whose count pass (tknnHaloSelect) marks the tile's boundary queries.
      phase 1 (max_rounds cap + 1, allow_unfinished): the interior queries in the own tree alone -- with the halo unset
              and with it already set, identically; boundary rows keep the sentinel, interior levels are the global ones
              up to cap and -1 above;
      phase 2: the boundary queries, halo = the complement's points in the tile's widened box; interior rows untouched;
      phase 3 (max_rounds 64): the queries still without a row, halo = the whole complement: every row and level global."""
    xyz, r0, ref = _replay(name, k)
    if (name, k) not in _LEVELS:
        _LEVELS[(name, k)] = trueknn_numpy(xyz, k, r0)["level"]
    lv = _LEVELS[(name, k)]
    cap = tile_sets.phase_cap(lv)
    eng = engines(name, "split")
    own, rest = eng.layout
    n = len(own)
    lay = tile_sets.phases(xyz, own, rest, r0, cap)
    boundary, near = lay["boundary"], lay["near"]
    interior = ~boundary
    lv_own = lv[own]
    capped = np.where(lv_own <= cap, lv_own, -1)
    assert boundary.any() and (interior & (lv_own <= cap)).any() and _has_ties(ref, own)
    kern = _lib.KERNEL_TEAM if k <= 64 else _lib.KERNEL_AUTO
    kw = dict(kernel=kern, max_rounds=cap + 1, allow_unfinished=True, want_levels=True)
    eng.set_halo(None, None)
    rows, counts = eng.halo_select(lay["peer_box"][None, :], [1], 2)
    assert counts[0] == 0
    # (the selection is the closed-box test of the numpy layout)
    assert sorted(_np(rows)[:, 3].view(np.int32).tolist()) == sorted(own[boundary].tolist())
    sentinel = _host(_sentinel(eng.device, n, k))
    results, tie_rows = [], 0
    for halo in (False, True):
        if halo:
            eng.set_halo(xyz[near], near)
        out = _sentinel(eng.device, n, k)
        r1 = eng.solve(k, r0, out=out, phase=1, **kw)
        got = _host(out)
        results.append(got)
        what = "%s k=%d cap=%d phase 1 (halo %s)" % (name, k, cap, "set" if halo else "unset")
        for field in ("idx", "dist", "intersections"):
            assert np.array_equal(got[field][boundary], sentinel[field][boundary]), (what, field, "boundary rows written")
        assert np.array_equal(got["levels"], np.where(interior, capped, -1)), what + ": levels"
        fin = np.nonzero(interior & (lv_own <= cap))[0]
        _check_rows({f: got[f][fin] for f in got}, ref, own[fin], what)
        assert r1["info"]["unfinished"] == int((interior & (lv_own > cap)).sum()) and r1["info"]["tie_rows_left"] == 0, what
        tie_rows += r1["info"]["tie_rows"]
    for field in results[0]:
        assert np.array_equal(results[0][field].view(np.uint8), results[1][field].view(np.uint8)), ("phase 1 read the halo", field)
    # phase 2 completes the outputs of the second phase-1 call (the halo already set)
    r2 = eng.solve(k, r0, out=out, phase=2, **kw)
    got = _host(out)
    what = "%s k=%d cap=%d phase 2" % (name, k, cap)
    for field in got:
        assert np.array_equal(got[field][interior].view(np.uint8), results[1][field][interior].view(np.uint8)), (what, field)
    assert np.array_equal(got["levels"], capped), what + ": levels"
    fin = np.nonzero(lv_own <= cap)[0]
    _check_rows({f: got[f][fin] for f in got}, ref, own[fin], what)
    assert r2["info"]["unfinished"] == int((boundary & (lv_own > cap)).sum()) and r2["info"]["tie_rows_left"] == 0, what
    tie_rows += r2["info"]["tie_rows"]
    # phase 3: the stragglers, over the whole complement
    eng.set_halo(xyz[rest], rest)
    try:
        r3 = eng.solve(k, r0, out=out, phase=3, kernel=kern, max_rounds=64, want_levels=True)
    finally:
        eng.set_halo(None, None)
    got = _host(out)
    what = "%s k=%d cap=%d phase 3" % (name, k, cap)
    assert np.array_equal(got["levels"], lv_own), what + ": levels"
    _check_rows(got, ref, own, what)
    assert r3["info"]["unfinished"] == 0 and r3["info"]["tie_rows_left"] == 0, what
    tie_rows += r3["info"]["tie_rows"]
    assert tie_rows > 0 if k <= 64 else tie_rows == 0


@pytest.mark.parametrize("name,k,kernel", [("cross", 3, "team"), ("lattice", 6, "team"), ("lattice", 16, "team"),
                                           ("lattice", 33, "team"), ("quantised", 48, "team"), ("lattice", 80, "auto")])
def test_start_radii_on_relabelled_tree(engines, name, k, kernel):
    """(e) per-query start radii (never with a halo) on the relabelled tree: rows are the replay's for each query's own
    start radius, and the tie pass still names neighbours by id."""
    import torch
    xyz, r0 = tile_sets.tie_set(name)
    eng = engines(name, "relabel")
    perm = eng.layout
    classes = np.float32([1.0, 0.75, 0.5]) if name == "cross" else np.float32([r0, 1.5 * r0, 2.5 * r0])
    local = np.random.default_rng(k).choice(classes, len(xyz)).astype(np.float32)
    radii = np.empty_like(local)
    radii[perm] = local
    ref = oracle.trueknn_per_query(xyz, k, radii)
    r = eng.solve(k, 1.0, kernel=KERNELS[kernel], start_radii=torch.from_numpy(local))
    what = "%s k=%d start radii" % (name, k)
    _check_rows(r, ref, perm, what)
    assert r["info"]["rounds"] == ref["rounds"], what
    _check_ties(r, ref, k, what)


def test_tile_surface_argument_contract(engines):
    """(f) what the tile options refuse, by code."""
    import torch
    xyz, r0, _ = _replay("lattice", 5)
    eng = engines("lattice", "split")
    own, rest = eng.layout
    box = tile_sets.phases(xyz, own, rest, r0, 1)["peer_box"][None, :]
    eng.halo_select(box, [1], 2)
    eng.build(xyz[own], own)  # a build drops the marks of the last count pass
    for phase in (1, 2):
        for k in (5, 65):
            with pytest.raises(_lib.TknnError) as e:
                eng.solve(k, r0, phase=phase, want_levels=True, allow_unfinished=True)
            assert e.value.code == -3, (phase, k)  # TKNN_E_STATE
    for k in (5, 65):
        with pytest.raises(_lib.TknnError) as e:
            eng.solve(k, r0, phase=3)  # without d_levels
        assert e.value.code == -1, k  # TKNN_E_ARG
    eng.halo_select(box, [1], 2)
    for kern in (_lib.KERNEL_LANE, _lib.KERNEL_WAVE):
        for phase in (1, 2, 3):
            with pytest.raises(_lib.TknnError) as e:
                eng.solve(5, r0, phase=phase, want_levels=True, allow_unfinished=True, kernel=kern)
            assert e.value.code == -5, (kern, phase)  # TKNN_E_UNSUPPORTED
    eng.set_halo(xyz[rest], rest)
    try:
        for k in (5, 65):
            with pytest.raises(_lib.TknnError) as e:
                eng.solve(k, r0, start_radii=torch.full((len(own),), r0))
            assert e.value.code == -5, k
    finally:
        eng.set_halo(None, None)
