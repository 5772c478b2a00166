"""tests/fpfh_spec.py held to what it promises, without a GPU: its histograms against their own invariants, the plane whose answer is
known in closed form, its neighbour sets against scipy's tree, csrc/fpfh_pair.h compiled for the host against its float64 features, and
the share of uncertain pairs on every input the GPU tests use."""
import numpy as np
import pytest

import fpfh_pair_host
import fpfh_spec as fs


@pytest.mark.parametrize("name", ["sphere1025", "cube1025", "dirty", "n17"])
def test_the_spec_against_itself(name):
    c = fs.case(name)
    counts, mem = c["hist"]["counts"], c["mem"]
    valid = counts[:, :11].sum(axis=1)
    assert np.array_equal(counts[:, 11:22].sum(axis=1), valid) and np.array_equal(counts[:, 22:].sum(axis=1), valid)
    assert valid.sum() + c["hist"]["skipped"] == c["hist"]["pairs"] == mem["lengths"].sum()
    spfh = fs.spfh64(counts)
    weighted = np.bincount(np.repeat(np.arange(len(valid)), mem["lengths"]), weights=(mem["d2"] > 0) * valid[mem["idx"]], minlength=len(valid)) > 0
    for self_term in (True, False):
        fpfh = fs.fpfh64(counts, mem, self_term)
        assert (fpfh >= 0).all() and np.isfinite(fpfh).all()
        for f in range(3):
            cols = slice(11 * f, 11 * f + 11)
            s = spfh[:, cols].sum(axis=1)
            assert np.allclose(s[valid > 0], 100.0, rtol=1e-12) and (s[valid == 0] == 0).all()
            want = 100.0 * weighted + (s if self_term else 0.0)  # a row some neighbour with a histogram blends into sums to 100, plus its own
            assert np.allclose(fpfh[:, cols].sum(axis=1), want, rtol=1e-12, atol=0)
    assert weighted.any() and (valid > 0).any()
    if name == "dirty":
        assert c["hist"]["skipped"] > 0 and (valid == 0).any()


@pytest.mark.parametrize("name", ["plane1025", "plane4200"])
def test_the_plane_is_known_in_closed_form(name):
    c = fs.case(name)
    counts, lengths = c["hist"]["counts"], c["mem"]["lengths"]
    assert c["hist"]["skipped"] == 0 and (c["hist"]["uncertain"] == 0).all(), "f1 = f2 = f3 = 0 on every pair, in the middle of a bin"
    want = np.zeros_like(counts)
    want[:, 5] = want[:, 16] = want[:, 27] = lengths
    assert np.array_equal(counts, want)
    full = np.zeros(counts.shape)
    full[lengths > 0, 5] = full[lengths > 0, 16] = full[lengths > 0, 27] = 100.0
    spfh = fs.spfh64(counts)
    assert np.array_equal(spfh == 0, full == 0) and np.allclose(spfh, full, rtol=1e-14, atol=0)  # (c * (100 / c) is 100 up to a rounding)
    has = np.bincount(np.repeat(np.arange(len(lengths)), lengths), weights=lengths[c["mem"]["idx"]] > 0, minlength=len(lengths)) > 0
    assert np.array_equal(has, lengths > 0)
    assert np.allclose(fs.fpfh64(counts, c["mem"], True), 2 * full, rtol=1e-13) and np.allclose(fs.fpfh64(counts, c["mem"], False), full, rtol=1e-13)
    # the fp32 pair function gives exactly 0 three times
    mem = c["mem"]
    src = np.repeat(np.arange(len(lengths)), lengths)
    dp = c["P"][mem["idx"]] - c["P"][src]
    valid, bins, feats = fpfh_pair_host.pairs(c["N"][src], c["N"][mem["idx"]], dp, mem["d2"], mem["d"])
    assert valid.all() and (feats == 0).all() and (bins == 5).all()


@pytest.mark.parametrize("name", ["sphere1025", "cube4200", "dirty"])
def test_neighbour_sets_agree_with_a_kd_tree(name):
    from scipy.spatial import cKDTree

    c = fs.case(name)
    P, mem, r = c["P"], c["mem"], float(c["r"])
    clean = np.nonzero(~np.isnan(P).any(axis=1))[0]
    tree = cKDTree(P[clean].astype(np.float64))
    wide, tight = tree.query_ball_point(P[clean].astype(np.float64), r * (1 + 1e-6)), tree.query_ball_point(P[clean].astype(np.float64), r * (1 - 1e-6))
    for at, i in enumerate(clean):
        row = set(mem["idx"][mem["offsets"][i]:mem["offsets"][i + 1]].tolist())
        assert i not in row
        assert {int(clean[j]) for j in tight[at]} - {int(i)} <= row <= {int(clean[j]) for j in wide[at]}
    dirty = np.nonzero(np.isnan(P).any(axis=1))[0]
    assert (mem["lengths"][dirty] == 0).all() and not np.isin(mem["idx"], dirty).any()


@pytest.mark.parametrize("name", fs.CASE_NAMES)
def test_the_host_build_of_the_pair_function_disagrees_only_on_uncertain_pairs(name):
    c = fs.case(name)
    mem, feat = c["mem"], c["feat"]
    src = feat["src"]
    dp = c["P"][mem["idx"]] - c["P"][src]
    valid, bins, _ = fpfh_pair_host.pairs(c["N"][src], c["N"][mem["idx"]], dp, mem["d2"], mem["d"])
    both = valid & feat["enters"]
    differs = (bins.T != feat["bins"]) & both[None, :]
    print("%s: %d pairs, %d bin disagreements, %d uncertain" % (name, len(src), int(differs.sum()), int(feat["uncertain"].sum())))
    assert not (differs & ~feat["uncertain"]).any(), "a bin differs on a pair the spec calls certain"
    one_sided = valid != feat["enters"]
    assert not (one_sided[None, :] & ~feat["uncertain"]).any(), "a pair enters on one side only and is not uncertain"


@pytest.mark.parametrize("name", fs.CASE_NAMES)
def test_uncertain_pairs_are_rare_on_every_gpu_case(name):
    c = fs.case(name)
    pairs = max(c["hist"]["pairs"], 1)
    share = c["feat"]["uncertain"].any(axis=0).sum() / pairs
    print("%s: %d pairs, uncertain share %.2e" % (name, c["hist"]["pairs"], share))
    assert share <= fs.UNCERTAIN_CAP
