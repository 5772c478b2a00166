"""The numpy definition of tknnFeatureMatch and tknnRansac (tests/global_spec.py) against what can be checked without a GPU: its
Kabsch, its draws, the header's sampler compiled for the host, the ctypes records against the header, and the cap -- how much of the
scenes the GPU tests use the spec alone cannot decide."""
import ctypes
import os
import subprocess

import numpy as np

import global_spec as gs
import ransac_sample_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kabsch_recovers_a_known_transform():
    rng = np.random.default_rng(0)
    for n in (3, 4, 50):
        T0 = gs.rigid(rng)
        s = rng.random((n, 3))
        p = s @ T0[:3, :3].T + T0[:3, 3]
        T, aux, ratio = gs.kabsch(s, p)
        assert np.abs(T - T0).max() < 1e-12 and ratio > 1e-3
        assert abs(np.linalg.det(T[:3, :3]) - 1) < 1e-12
    # a reflection is not taken: mirrored points give a proper rotation still
    s = rng.random((4, 3))
    T, _, _ = gs.kabsch(s, s * np.array([1.0, 1.0, -1.0]))
    assert np.linalg.det(T[:3, :3]) > 0.999
    # collinear points: degenerate
    sc = gs.collinear_scene()
    T, _, ratio = gs.kabsch(sc["S"], sc["P"][:3])
    assert T is None and ratio < 2.0 ** -50


def test_match_spec_on_a_case_done_by_hand():
    A = np.float32([[0, 0], [3, 0], [np.nan, 0]])
    B = np.float32([[1, 0], [0, 1], [np.inf, 0], [-1, 0]])
    best, b1, b2 = gs.match(A, B)
    assert best.tolist() == [0, 0, -1] and b1.tolist()[:2] == [1.0, 4.0] and b2.tolist()[:2] == [1.0, 10.0] and np.isinf(b1[2]) and np.isinf(b2[2])
    best, b1, b2 = gs.match(A[:2], B[:1])
    assert best.tolist() == [0, 0] and np.isinf(b2).all()
    rows = gs.fpfh_like(np.random.default_rng(1), 50)
    assert (rows >= 0).all() and np.allclose(rows.reshape(50, 3, 11).sum(axis=2), 100, atol=1e-3) and (rows == 0).mean() > 0.3


def test_draws_are_distinct_and_in_range():
    for n in (3, 4):
        for c in (64, 200, 100000):
            idx, ok = gs.samples(gs.TRIAL_SEED, np.arange(4096), n, c)
            assert ok.all(), "no DUPLICATE for c >= 64 over 4096 trials of the committed seed"
            assert (idx >= 0).all() and (idx < c).all()
            srt = np.sort(idx, axis=1)
            assert (srt[:, 1:] != srt[:, :-1]).all()
    idx, ok = gs.samples(gs.TRIAL_SEED, np.arange(4096), 3, 3)
    assert 0 < (~ok).sum() < 4096, "three records: some trials cannot draw three distinct ones in eight tries"
    assert all(sorted(r) == [0, 1, 2] for r in idx[ok])
    _, ok = gs.samples(gs.TRIAL_SEED, np.arange(64), 3, 2)
    assert not ok.any()


def test_the_headers_sampler_gives_the_specs_indices():
    rng = np.random.default_rng(2)
    count = 4000
    seed = rng.integers(0, 2 ** 32, size=count, dtype=np.uint64).astype(np.uint32)
    trial = rng.integers(0, 2 ** 31, size=count).astype(np.uint32)
    n = rng.integers(3, 5, size=count).astype(np.int32)
    c = np.where(rng.random(count) < 0.2, rng.integers(1, 8, size=count), rng.integers(8, 2 ** 31 - 2, size=count)).astype(np.uint32)
    idx, ok = ransac_sample_host.samples(seed, trial, n, c)
    for i in range(count):
        want, want_ok = gs.samples(seed[i], trial[i:i + 1], int(n[i]), int(c[i]))
        assert bool(want_ok[0]) == bool(ok[i]), i
        if ok[i]:
            assert want[0].tolist() == idx[i, :n[i]].tolist(), i
    assert 0 < (~ok).sum() < count


def test_ctypes_records_have_the_header_layout(tmp_path):
    from owlraytracing_amd import _global_lib as gl

    pairs = {"tknnFeatureMatchOptions": gl.FeatureMatchOptions, "tknnFeatureMatchInfo": gl.FeatureMatchInfo, "tknnRansacOptions": gl.RansacOptions,
             "tknnRansacInfo": gl.RansacInfo}
    mirrors = {c for c in vars(gl).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and getattr(c, "_fields_", None)}
    assert mirrors == set(pairs.values())
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn_global.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = 0
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, what, value = line.split()
        if what == "size":
            assert ctypes.sizeof(pairs[cname]) == int(value), cname
        else:
            assert getattr(pairs[cname], what).offset == int(value), (cname, what)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in pairs.values())
    text = open(os.path.join(ROOT, "include", "owlknn_global.h")).read()
    assert "#define TKNN_RANSAC_BATCH %d" % gl.RANSAC_BATCH in text and "#define TKNN_MATCH_MAX_D %d" % gl.MATCH_MAX_D in text
    for value, name in enumerate(gl.STATUS):
        assert "#define TKNN_RANSAC_%s %d" % (name.upper(), value) in text


def test_the_cap_on_what_the_spec_cannot_decide():
    """For every RANSAC scene of the GPU tests: at most 1 % of the (scored trial, record) combinations are uncertain, at most 1 % of
    the trials are excluded from the status comparison, and the scenes do reach every status the tests look for."""
    for n in (3, 4):
        sc, tr = gs.scene_trials(n)
        scored = tr["status"] == gs.OK
        assert scored.sum() >= 5, "the scene must score some trials"
        assert tr["uncertain"][scored].sum() <= 0.01 * scored.sum() * len(sc["pairs"])
        assert tr["excluded"].sum() <= 0.01 * len(tr["status"])
        assert (tr["status"] == gs.EDGE).any() and (tr["status"] == gs.FAR).any()
        assert tr["E"][scored].max() < 1e-4, "the bound stays far below max_dist"
        best = np.argmax(np.where(scored, tr["certain"], -1))
        assert tr["certain"][best] >= 0.5 * len(sc["pairs"]), "the best trial finds the planted motion"
    sc = gs.collinear_scene()
    tr = gs.run_trials(sc["S"], sc["P"], sc["pairs"], 3, gs.MAX_DIST, 0.9, gs.TRIAL_SEED, np.arange(256))
    assert set(tr["status"]) == {gs.DUPLICATE, gs.DEGENERATE} and not tr["excluded"].any()
