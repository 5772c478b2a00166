"""tests/fps_spec.py checked against itself on the CPU: the cases are what they claim, the pruned restatement of tknnFps picks the
brute-force samples on every case, over trees rebuilt by tests/lbvh_spec.py, and prunes what its design requires."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_spec as bs  # noqa: E402
import fps_spec as fs  # noqa: E402
import lbvh_spec as ls  # noqa: E402


def replay(P, row, names=None):
    """Follows one brute-force row over the points P of its cloud: per sample after the first, how many unchosen points held the
    largest D when it was chosen; asserts that each sample is one of them and the one of the smallest name."""
    P = fs.pad_to_3d(np.asarray(P, np.float32))
    names = np.arange(len(P)) if names is None else np.asarray(names)
    at = {int(v): i for i, v in enumerate(names)}
    D = np.full(len(P), np.inf, np.float32)
    alive = np.ones(len(P), bool)
    ties = []
    for t, name in enumerate(row):
        i = at[int(name)]
        assert alive[i], "a point is sampled twice"
        if t:
            top = D[alive].max()
            tied = np.flatnonzero(alive & (D == top))
            assert D[i] == top and names[i] == names[tied].min()
            ties.append(len(tied))
        D = np.minimum(D, fs.d2_to(P, P[i]))
        alive[i] = False
    return np.array(ties)


def test_lattice_choices_are_ties():
    P = fs.lattice_case()
    want = fs.brute(P, 200)
    ties = replay(P, want["idx"][0])
    # (the first few samples are the lattice's corners, alone at their distance; from then on the name decides)
    assert len(ties) == 199 and (ties >= 2).sum() >= 150 and ties.max() >= 100, "most choices on the lattice are between equal distances"
    d = want["dist"][0]
    assert np.isinf(d[0]) and (np.diff(d[1:]) <= 0).all(), "the covering radius never grows"


def test_duplicates_come_last_in_name_order():
    P = fs.duplicates_case()
    assert len(np.unique(P, axis=0)) == 512
    want = fs.brute(P, 1024)
    idx, d = want["idx"][0], want["dist"][0]
    assert want["counts"][0] == 1024 and sorted(idx) == list(range(1024))
    assert len(np.unique(P[idx[:512]], axis=0)) == 512 and (d[1:512] > 0).all()
    assert (d[512:] == 0).all() and (np.diff(idx[512:]) > 0).all()
    replay(P, idx)


def test_counts_starts_and_padding():
    P, batch = fs.nan_case()
    clean = ~np.isnan(P).any(axis=1)
    sizes = np.array([(clean & (batch == b)).sum() for b in range(3)])
    nan_row, other = int(np.flatnonzero(~clean)[0]), int(np.flatnonzero(clean & (batch == 1))[0])
    own = int(np.flatnonzero(clean & (batch == 0))[5])
    want = fs.brute(P, 50, batch=batch, num=[0, 1, 10**6], start_rows=[own, nan_row, 800])
    assert want["counts"].tolist() == [0, 1, 50] and want["bad_starts"] == 2
    assert (want["idx"][0] == -1).all() and np.isinf(want["dist"]).sum() == 50 + (1 + 49) + 1
    want = fs.brute(P, 400, batch=batch, start_rows=[own, other, -1])
    assert want["counts"].tolist() == np.minimum(sizes, 400).tolist() and want["bad_starts"] == 0
    assert want["idx"][0, 0] == own and want["idx"][1, 0] == other
    assert want["idx"][2, 0] == np.flatnonzero(clean & (batch == 2))[0], "the default start: the smallest name"
    assert not np.isin(np.flatnonzero(~clean), want["idx"]).any(), "a NaN point is never sampled"
    for b in range(3):
        replay(P[clean & (batch == b)], want["idx"][b, : want["counts"][b]], np.flatnonzero(clean & (batch == b)))


def plain(P, S, ids=None, **kw):
    tree = ls.build_points(fs.pad_to_3d(np.asarray(P, np.float32)), ids=ids)
    return fs.brute(P, S, ids=ids, **kw), fs.visited_blocks(tree, S, **kw)


def batched(P, batch, B, S, **kw):
    tree = bs.build_points(P, batch, B)
    return fs.brute(P, S, batch=batch, num_batches=B, **kw), fs.visited_blocks(tree, S, starts=tree["starts"], **kw)


@pytest.mark.parametrize("case", ["n1", "n6", "n6_clipped", "n17", "lattice", "duplicates", "ids", "planar", "uniform"])
def test_pruned_restatement_picks_the_brute_force_samples(case):
    ids = None
    if case in ("n1", "n6", "n6_clipped", "n17"):
        P, S = fs.uniform_case(int(case[1:].split("_")[0]), 710), 10 if case == "n6_clipped" else int(case[1:].split("_")[0])
    elif case == "lattice":
        P, S = fs.lattice_case(), 200
    elif case == "duplicates":
        P, S = fs.duplicates_case(), 1024
    elif case == "ids":
        (P, ids), S = fs.ids_case(), 300
    elif case == "planar":
        P, S = fs.planar_case(), 200
    else:
        P, S = fs.uniform_case(2000, 711), 500
    want, got = plain(P, S, ids=ids)
    assert np.array_equal(got["idx"], want["idx"]) and np.array_equal(got["counts"], want["counts"])
    assert got["visits"][0] <= got["touching"][0] * want["counts"][0]


def test_pruned_restatement_on_batched_trees():
    P, batch = fs.tiny_clouds_case()
    want, got = batched(P, batch, 3, 8)
    assert np.array_equal(got["idx"], want["idx"]) and want["counts"].tolist() == [6, 0, 4]
    P, batch = fs.straddle_case()
    B = len(fs.STRADDLE_SIZES)
    start_rows = np.full(B, -1)
    start_rows[5] = int(np.flatnonzero(batch == 5)[77])
    want, got = batched(P, batch, B, 64, start_rows=start_rows)
    assert np.array_equal(got["idx"], want["idx"]) and want["counts"].tolist() == [5, 40, 1, 16, 17, 64]
    assert got["touching"][:5].tolist() == [1, 3, 1, 2, 2], "the small clouds straddle blocks"
    P, batch = fs.nan_case()
    want, got = batched(P, batch, 3, 100, num=[100, 7, 0])
    assert np.array_equal(got["idx"], want["idx"]) and np.array_equal(got["counts"], want["counts"])
    same = fs.visited_blocks(bs.build_points(P, batch, 3), 100, starts=bs.build_points(P, batch, 3)["starts"], num=[100, 7, 0], prune=False)
    assert np.array_equal(same["idx"], want["idx"]) and np.array_equal(same["visits"], same["touching"] * want["counts"])


def test_the_rule_prunes_three_quarters_on_uniform_4096():
    """A condition of the design: on 4096 uniform points and 1024 samples the visited blocks hold at most a quarter of the
    points brute force touches (the restatement measured 0.05 - 0.06 of them when the rule was proposed)."""
    from owlraytracing_amd import datasets

    P = datasets.uniform3d(4096, seed=5)
    want, got = plain(P, 1024)
    assert np.array_equal(got["idx"], want["idx"])
    share = 16 * int(got["visits"][0]) / (4096 * 1024)
    print("share of brute force's point updates: %.4f" % share)
    assert 16 * int(got["visits"][0]) * 4 <= 4096 * 1024
