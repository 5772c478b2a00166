"""What tknnFeatureMatch and tknnRansac (include/owlknn_global.h) refuse, one fault per row and in the header's order, that the
message names the call and the field, and that a refused call writes nothing, neither outputs nor info."""
import ctypes

import numpy as np
import pytest

import global_spec as gs

pytestmark = pytest.mark.gpu

ARG = -1
TOO_MANY = 2 ** 31 - 1


def test_feature_match_error_codes_in_order():
    import torch

    from owlraytracing_amd import _global_lib as gl
    from owlraytracing_amd.trueknn import TrueKNN

    lib = gl.load()
    eng = TrueKNN(device=0)  # no tree
    dev = eng.device
    m, n, D, guard = 70, 90, 33, 64
    rng = np.random.default_rng(0)
    A, B = rng.random((m, D), dtype=np.float32), rng.random((n, D), dtype=np.float32)
    src, tgt = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    bufs = {"d_best": torch.full((m + guard,), -7, dtype=torch.int32, device=dev), "d_best_d2": torch.full((m + guard,), -7.0, dtype=torch.float32, device=dev),
            "d_second_d2": torch.full((m + guard,), -7.0, dtype=torch.float32, device=dev)}
    info = gl.FeatureMatchInfo()

    def call(handle=None, options=True, with_info=True, outputs=tuple(bufs), **kw):
        o = gl.FeatureMatchOptions()
        o.m, o.n, o.D, o.d_source, o.d_target = m, n, D, src.data_ptr(), tgt.data_ptr()
        for name in outputs:
            setattr(o, name, bufs[name].data_ptr())
        for name, v in kw.items():
            setattr(o, name, v)
        info.pair_tests, info.chunks, info.solve_ms = 99, 98, 97.0
        rc = lib.tknnFeatureMatch(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info) if with_info else None, None)
        assert rc == 0 or (info.pair_tests == 99 and info.chunks == 98 and info.solve_ms == 97.0), "a refused call leaves the info alone"
        return rc

    def untouched(but=()):
        return all(bool((b == -7).all()) for name, b in bufs.items() if name not in but)

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnFeatureMatch: "), t
        return t

    # 1. missing pointers, no output -- before any value
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(with_info=False) == ARG and "info" in text()
    assert call(with_info=False, D=0) == ARG and "info" in text()
    assert call(outputs=()) == ARG and "no output" in text()
    assert call(outputs=(), d_source=None) == ARG and "no output" in text()
    assert call(d_source=None) == ARG and "d_source" in text()
    assert call(d_source=None, d_target=None) == ARG and "d_source" in text()
    assert call(d_target=None, D=0) == ARG and "d_target" in text()
    # 2. the values, in the header's order
    for bad in (0, -1, 65, 1 << 20):
        assert call(D=bad) == ARG and "D must" in text()
        assert call(D=bad, m=-1) == ARG and "D must" in text()
    for bad in (-1, TOO_MANY):
        assert call(m=bad) == ARG and "<= m <" in text()
        assert call(m=bad, n=-1) == ARG and "<= m <" in text()
        assert call(n=bad, flags=1) == ARG and "<= n <" in text()
    for bad in (1, 8, 0x80000000):
        assert call(flags=bad) == ARG and "flag" in text()
    assert untouched(), "a refused call writes nothing"
    # 3. m = 0: a zeroed info, nothing written, NULL rows allowed; n = 0: every row without a match
    assert call(m=0, d_source=None) == 0 and info.pair_tests == 0 and info.chunks == 0 and info.solve_ms == 0 and untouched()
    assert call(n=0, d_target=None) == 0 and info.pair_tests == 0 and info.chunks == 0
    assert (bufs["d_best"][:m] == -1).all() and torch.isinf(bufs["d_best_d2"][:m]).all() and torch.isinf(bufs["d_second_d2"][:m]).all()
    # the call itself; nothing is written behind the m rows, and every output asked alone gives the same bits
    best, b1, b2 = gs.match(A, B)
    assert call() == 0 and info.pair_tests == m * n and info.solve_ms >= info.match_ms > 0 and info.merge_ms > 0
    everything = {name: b.clone() for name, b in bufs.items()}
    assert np.array_equal(everything["d_best"][:m].cpu().numpy(), best) and np.array_equal(everything["d_best_d2"][:m].cpu().numpy(), b1)
    assert np.array_equal(everything["d_second_d2"][:m].cpu().numpy(), b2)
    for name, b in bufs.items():
        assert (b[m:] == -7).all(), name
    for name in bufs:
        for b in bufs.values():
            b.fill_(-7)
        assert call(outputs=(name,)) == 0 and untouched(but=(name,))
        assert torch.equal(bufs[name].view(torch.int32), everything[name].view(torch.int32)), name
    eng.close()


def test_ransac_error_codes_in_order():
    import torch

    from owlraytracing_amd import _global_lib as gl
    from owlraytracing_amd.trueknn import TrueKNN

    lib = gl.load()
    eng = TrueKNN(device=0)  # no tree
    dev = eng.device
    sc, _ = gs.scene_trials(3)
    ms, mt, c, trials, guard = len(sc["S"]), len(sc["P"]), len(sc["pairs"]), 300, 64
    src, tgt, pairs = (torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev) for k in ("S", "P", "pairs"))
    bufs = {"d_inlier_mask": torch.full((c + guard,), 0xF9, dtype=torch.uint8, device=dev),
            "d_trial_status": torch.full((trials + guard,), -7, dtype=torch.int32, device=dev),
            "d_trial_inliers": torch.full((trials + guard,), -7, dtype=torch.int32, device=dev)}
    info = gl.RansacInfo()

    def call(handle=None, options=True, with_info=True, **kw):
        o = gl.RansacOptions()
        o.ms, o.mt, o.c, o.d_source, o.d_target, o.d_pairs = ms, mt, c, src.data_ptr(), tgt.data_ptr(), pairs.data_ptr()
        o.ransac_n, o.max_dist, o.edge_similarity, o.max_trials, o.confidence, o.seed, o.refit_rounds = 3, gs.MAX_DIST, 0.9, trials, 1.0, gs.TRIAL_SEED, 1
        for name, b in bufs.items():
            setattr(o, name, b.data_ptr())
        for name, v in kw.items():
            setattr(o, name, v)
        info.best_trial, info.inliers, info.solve_ms, info.transform[5] = 99, 98, 97.0, 96.0
        rc = lib.tknnRansac(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info) if with_info else None, None)
        assert rc == 0 or (info.best_trial == 99 and info.inliers == 98 and info.solve_ms == 97.0 and info.transform[5] == 96.0), "a refused call leaves the info alone"
        return rc

    def untouched():
        return bool((bufs["d_inlier_mask"] == 0xF9).all()) and bool((bufs["d_trial_status"] == -7).all()) and bool((bufs["d_trial_inliers"] == -7).all())

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnRansac: "), t
        return t

    # 1. missing pointers -- before any value
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(with_info=False) == ARG and "info" in text()
    assert call(with_info=False, ransac_n=5) == ARG and "info" in text()
    assert call(d_source=None, ransac_n=5) == ARG and "d_source" in text()
    assert call(d_source=None, d_target=None) == ARG and "d_source" in text()
    assert call(d_target=None, d_pairs=None) == ARG and "d_target" in text()
    assert call(d_pairs=None, max_dist=0.0) == ARG and "d_pairs" in text()
    # 2. the values, in the header's order: each fault with the next one along
    faults = [("ransac_n", (2, 5, 0, -3), "ransac_n"), ("max_dist", (0.0, -1.0, float("nan"), float("inf")), "max_dist"),
              ("edge_similarity", (-0.1, 1.5, float("nan")), "edge_similarity"), ("confidence", (0.0, -0.5, 1.0001, float("nan")), "confidence"),
              ("max_trials", (0, -4), "max_trials"), ("refit_rounds", (-1, 9), "refit_rounds"), ("ms", (-1, TOO_MANY), "<= ms <"), ("mt", (-1, TOO_MANY), "<= mt <"),
              ("c", (-1, TOO_MANY), "<= c <"), ("flags", (1, 0x80000000), "flag")]
    for i, (field, values, says) in enumerate(faults):
        later = {faults[i + 1][0]: faults[i + 1][1][0]} if i + 1 < len(faults) else {}
        for v in values:
            assert call(**{field: v}) == ARG and says in text(), (field, v, text())
            assert call(**dict(later, **{field: v})) == ARG and says in text(), (field, v, text())
    # 3. a pair row out of range: found on the device, and still nothing is written
    for bad in ([0, mt], [ms, 0], [-1, 0], [0, -1]):
        wrong = pairs.clone()
        wrong[c - 1] = torch.tensor(bad, dtype=torch.int32)
        assert call(d_pairs=wrong.data_ptr()) == ARG and "d_pairs" in text()
    assert untouched(), "a refused call writes nothing"
    # c < ransac_n is no error
    assert call(c=2) == 0 and info.best_trial == -1 and info.trials_run == 0 and info.inliers == 0
    assert (bufs["d_trial_status"][:trials] == -1).all() and (bufs["d_inlier_mask"][:2] == 0).all() and (bufs["d_inlier_mask"][2:] == 0xF9).all()
    # the call itself; nothing is written behind the rows
    assert call() == 0 and info.best_trial >= 0 and info.trials_run == trials and info.inliers >= 0.5 * c
    assert info.solve_ms > 0 and info.sample_ms > 0 and info.score_ms > 0 and info.refit_ms > 0
    assert (bufs["d_inlier_mask"][c:] == 0xF9).all() and int(bufs["d_inlier_mask"][:c].sum()) == info.inliers
    assert (bufs["d_trial_status"][trials:] == -7).all() and (bufs["d_trial_inliers"][trials:] == -7).all()
    assert (bufs["d_trial_status"][:trials] >= 0).all()
    eng.close()


def test_the_wrappers_pass_the_codes_on():
    from owlraytracing_amd._lib import TknnError
    from owlraytracing_amd.trueknn import TrueKNN

    eng = TrueKNN(device=0)
    sc, _ = gs.scene_trials(3)
    with pytest.raises(TknnError) as err:
        eng.match_features(np.zeros((3, 65), np.float32), np.zeros((4, 65), np.float32))
    assert err.value.code == ARG and str(err.value).count("tknnFeatureMatch") == 1 and "D must" in str(err.value)
    with pytest.raises(ValueError):
        eng.match_features(np.zeros((3, 5), np.float32), np.zeros((4, 6), np.float32))
    for kw, says in ((dict(ransac_n=2), "ransac_n"), (dict(max_dist=0.0), "max_dist"), (dict(confidence=0.0), "confidence"), (dict(refit_rounds=9), "refit_rounds")):
        args = dict(max_dist=gs.MAX_DIST)
        args.update(kw)
        with pytest.raises(TknnError) as err:
            eng.ransac(sc["S"], sc["P"], sc["pairs"], **args)
        assert err.value.code == ARG and says in str(err.value) and str(err.value).count("tknnRansac") == 1
    eng.close()
