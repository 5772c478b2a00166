"""tests/team_lanes_spec.py without a GPU: the claim under t_sorted_row's one-word fast path (exhaustively), the specification of
every op against brute force -- Python's sorted on tuples, a scalar insertion list after KList::insert, scalar float32 loops --
the model of the path decision against the table of the boundary cases, and that the generated cases are what the case table of
tests/test_team_lanes_gpu.py says.  The entry point's header, binding and refusals: tests/test_debug_expectations.py."""
import math
import os
import struct
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import team_lanes_spec as ts  # noqa: E402

U32, F32 = np.uint32, np.float32
SORTS = (ts.SORT16, ts.CLEAN16, ts.SORT16_U32, ts.SORT16_3, ts.CLEAN16_3)


def test_roots_of_squares_two_truncated_words_apart_differ():
    """The fast path orders two squares by their words without the last four bits when those are two or more apart.  That is the
    order of the (root, id) keys only if the ROUNDED roots differ too: for every truncated word T the largest square of T and the
    smallest of T + 2 -- 17 ulps apart -- must have different roots.  Every T below 0x7f7ffff0 >> 4: 133 693 439 pairs, the last two
    with +inf as the larger square."""
    top = ts.TOP_WORD >> 4
    assert top == 133693439
    bad = 0
    for first in range(0, top, 1 << 23):
        T = np.arange(first, min(first + (1 << 23), top), dtype=np.uint64)
        lo, hi = (T * np.uint64(16) + np.uint64(15)).astype(U32), ((T + np.uint64(2)) * np.uint64(16)).astype(U32)
        bad += int((~(np.sqrt(lo.view(F32)) < np.sqrt(hi.view(F32)))).sum())
    print("root ordering: %d pairs, %d counter-examples" % (top, bad))
    assert bad == 0


def test_no_four_floats_share_a_rounded_root():
    """(sampled) the pre-image of one rounded root spans at most three floats, so squares sixteen or more ulps apart never tie"""
    rng = np.random.default_rng(77)
    x = np.concatenate([ts.rand_d2(rng, 1 << 22, specials=False), np.arange(0, 1 << 16, dtype=U32), np.arange(ts.TOP_WORD - (1 << 16), ts.TOP_WORD, dtype=U32)])
    assert (ts.root_bits(x) < ts.root_bits(x + U32(3))).all()
    pairs = ts.equal_root_pairs()
    assert len(pairs) == 48 and all(ts.root_bits(U32(v)) == ts.root_bits(U32(v + 1)) for v in pairs)
    assert all(v & 15 != 15 for v in pairs[:24]) and all(v & 15 == 15 for v in pairs[24:]), "inside a truncated word, and across two"


# ---- brute force ----------------------------------------------------------------------------------------------------------------
def _f(word):
    return struct.unpack("<f", struct.pack("<I", int(word)))[0]


def _w(value):
    return struct.unpack("<I", struct.pack("<f", value))[0]


def _root(word):  # the double root rounded once more: exact for float32 (53 >= 2 * 24 + 2)
    return _w(math.sqrt(_f(word)))


def _brute_sort(x):
    nw = x.shape[0]
    keys = sorted(tuple(int(x[w, l]) for w in range(nw)) for l in range(16))
    return np.array(keys, U32).T


def _brute_row(x):
    keys = [(_root(x[0, l]), int(x[1, l])) for l in range(16) if x[2, l]]
    keys = sorted(keys + [(ts.EMPTY_WORD, 0)] * (16 - len(keys)))  # (the root of an infinite square lies beyond the empty key)
    return np.array(keys, U32).T


def _brute_merge(x, n):
    """KList::insert, one candidate at a time; left_out as the list tracks it, kept only if `full`"""
    K = 16 * n
    lst = [(int(x[j // 16, j % 16]), int(x[n + j // 16, j % 16])) for j in range(K)]
    fill, left, full = int(x[2 * n + 4, 0]), int(x[2 * n + 5, 0]), bool(x[2 * n + 6, 0])
    for c in range(fill):
        key = (_root(x[2 * n + 2 * (c // 16), c % 16]), int(x[2 * n + 1 + 2 * (c // 16), c % 16]))
        if key < lst[K - 1]:
            out = lst[K - 1][0]
            j = K - 1
            while j > 0 and key < lst[j - 1]:
                lst[j] = lst[j - 1]
                j -= 1
            lst[j] = key
        else:
            out = key[0]
        if full:
            left = min(left, out)
    res = np.zeros((2 * n + 1, 16), U32)
    for j, (d, i) in enumerate(lst):
        res[j // 16, j % 16], res[n + j // 16, j % 16] = d, i
    res[2 * n] = min(left, ts.EMPTY_WORD)
    return res


def _brute_straddle(d, r0, r_last, qmax, span):
    d, r, r_last, qmax, span = F32(d), F32(r0), F32(r_last), F32(qmax), F32(span)
    while True:
        mg = F32(F32(qmax + F32(F32(2.0) * r)) * F32(4.76837158203125e-07))
        if d <= F32(F32(r - mg) * F32(0.99999)):
            return False
        if d <= F32(F32(r + mg) * span):
            return True
        if not r < r_last:
            return True
        r = F32(r * F32(2.0))


def _brute_row_ties(x, n):
    K = 16 * n
    res = np.zeros((2, 16), U32)
    e = [int(x[j // 16, j % 16]) for j in range(K)]
    for j in range(K):
        l = j % 16
        left, full, k, look = int(x[n, l]), bool(x[n + 1, l]), int(x[n + 2, l]), bool(x[n + 9, l])
        qmax = max(abs(_f(x[n + 3 + a, l])) for a in range(3))
        with_before = 1 <= j <= k and e[j] == e[j - 1]
        with_left = j == K - 1 and full and left == e[j]
        if (with_before or with_left) and look and _brute_straddle(_f(e[j]), _f(x[n + 6, l]), _f(x[n + 7, l]), qmax, _f(x[n + 8, l])):
            res[0, l] = 1
            if j == k or with_left:
                res[1, l] = 1
    return res


def _brute_first_level(x):
    res = np.zeros((1, 16), U32)
    for l in range(16):
        p, q = [F32(_f(x[a, l])) for a in range(3)], [F32(_f(x[3 + a, l])) for a in range(3)]
        rr, level = F32(_f(x[6, l])), min(max(int(np.int32(x[7, l])), 0), 64)
        res[0, l] = level
        for lvl in range(level):
            if all(F32(p[a] - rr) <= q[a] <= F32(p[a] + rr) for a in range(3)):
                res[0, l] = lvl
                break
            rr = F32(rr * F32(2.0))
    return res


def _brute_wave(op, variant, inp, t):
    """REDUCE and MOVES for team t, which see their wave: plain Python over the wave's 64 lanes (zero words for missing teams)"""
    first = t // 4 * 4
    wave = np.zeros((4, inp.shape[1], 16), U32)
    wave[:min(4, inp.shape[0] - first)] = inp[first:first + 4]
    lanes = [[int(wave[s, w, l]) for s in range(4) for l in range(16)] for w in range(inp.shape[1])]
    mine = range(16 * (t & 3), 16 * (t & 3) + 16)
    if op == ts.REDUCE:
        v = [lanes[0][l] for l in mine]
        fl = [x for x in (_f(w) for w in v) if not math.isnan(x)]
        wave_fl = [x for x in (_f(w) for w in lanes[0]) if not math.isnan(x)]
        res = np.zeros((8, 16), U32)
        res[ts.R_SUM_U32] = sum(v) & 0xFFFFFFFF
        res[ts.R_MIN_F32], res[ts.R_MAX_F32], res[ts.R_MIN_U32] = _w(min(fl)), _w(max(fl)), min(v)
        res[ts.R_WAVE_MAX], res[ts.R_WAVE_SUM_LO], res[ts.R_WAVE_SUM_HI] = _w(max(wave_fl)), sum(lanes[0]) & 0xFFFFFFFF, sum(lanes[0]) >> 32
        return res
    res = np.zeros((15, 16), U32)
    v, src, bit, acc = lanes
    for l in range(16):
        me = mine[0] + l
        for word, other in ((ts.M_XOR4, l ^ 4), (ts.M_DPP_B1, l ^ 1), (ts.M_DPP_1B, (l & 12) + 3 - (l & 3)), (ts.M_DPP_4E, l ^ 2),
                            (ts.M_DPP_141, (l & 8) + 7 - (l & 7)), (ts.M_DPP_140, 15 - l), (ts.M_DPP_128, (l + 8) % 16), (ts.M_DPP_121, (l + 15) % 16),
                            (ts.M_LANE_READ, src[me] & 15)):
            res[word, l] = v[mine[0] + other]
        res[ts.M_SHR1, l] = v[me - 1] if l else 0
        res[ts.M_RANK, l] = sum(1 for b in bit[:me] if b)
        res[ts.M_COUNT, l] = res[ts.M_COUNT_KEEP, l] = (acc[me] + (1 if bit[me] else 0)) & 0xFFFFFFFF
        res[ts.M_TEAM_ANY, l] = int(any(bit[m] for m in mine))
        res[ts.M_BCAST, l] = v[variant]
    return res


def _brute(op, variant, inp, t):
    x = inp[t]
    if op in SORTS:
        return _brute_sort(x)
    if op == ts.SORTED_ROW:
        return _brute_row(x)
    if op == ts.MERGE:
        return _brute_merge(x, variant)
    if op == ts.KTH:
        return np.array([[int(x[(int(x[variant, l]) - 1) // 16, (int(x[variant, l]) - 1) % 16]) for l in range(16)]], U32)
    if op == ts.ROW_TIES:
        return _brute_row_ties(x, variant)
    if op == ts.STRADDLE:
        return np.array([[int(_brute_straddle(*[_f(x[w, l]) for w in range(5)])) for l in range(16)]], U32)
    if op == ts.FIRST_LEVEL:
        return _brute_first_level(x)
    return _brute_wave(op, variant, inp, t)


def _classes(op, variant):
    """{class: input} of an op, every class the GPU test runs"""
    if op in SORTS:
        return ts.sort_cases(op)
    if op == ts.SORTED_ROW:
        return {"random": ts.row_random(), "duplicates": ts.row_duplicates(), "boundary": ts.row_boundary()[0], "have_masks": ts.row_have_masks()}
    if op == ts.MERGE:
        return {"merge": ts.merge_cases(variant)[0]}
    if op == ts.REDUCE:
        return ts.reduce_cases()
    return {"random": ts.random_cases(op, variant)}


@pytest.mark.parametrize("op,variant", [(op, v) for op in range(13) for v in (ts.MOVES_BCAST_LANES if op == ts.MOVES else ts.variants(op))],
                         ids=lambda x: str(x))
def test_spec_against_brute_force(op, variant):
    """every op and class at a handful of teams spread over the class (MERGE: 60, its table has 560 to 980 rows)"""
    with np.errstate(over="ignore", invalid="ignore"):
        for name, inp in _classes(op, variant).items():
            assert inp.dtype == U32 and inp.shape[1:] == (ts.words(op, variant)[0], 16) and 64 <= inp.shape[0] <= 4096, (ts.OP_NAMES[op], name, inp.shape)
            want = ts.expected(op, variant, inp)
            assert want.dtype == U32 and want.shape == (inp.shape[0], ts.words(op, variant)[1], 16)
            picks = np.unique(np.linspace(0, inp.shape[0] - 1, 60 if op == ts.MERGE else 12).astype(int))
            for t in picks:
                got = _brute(op, variant, inp, t)
                if op == ts.REDUCE:  # the float sum has a bound, not a word
                    total, bound = ts.fsum_bound(inp[t:t + 1])
                    exact = math.fsum(_f(w) for w in inp[t, 0])
                    assert name == "words" or (abs(total[0] - exact) <= 2.0 ** -29 * bound[0] and abs(float(ts.f32(want[t, ts.R_SUM_F32, :1])[0]) - exact) <= bound[0])
                    got[ts.R_SUM_F32] = want[t, ts.R_SUM_F32]
                assert np.array_equal(got, want[t]), (ts.OP_NAMES[op], variant, name, int(t))
        for count in ts.TEAM_COUNTS:  # the wave-wide words with teams missing from the last wave
            if op in (ts.REDUCE, ts.MOVES):
                inp = ts.random_cases(op, variant)[:count]
                want = ts.expected(op, variant, inp)
                got = _brute(op, variant, inp, count - 1)
                got[ts.R_SUM_F32 if op == ts.REDUCE else 0] = want[count - 1, ts.R_SUM_F32 if op == ts.REDUCE else 0]
                assert np.array_equal(got, want[count - 1]), (ts.OP_NAMES[op], variant, count)


def test_small_integers_sum_exactly_in_any_order():
    inp = ts.reduce_cases()["small_integers"]
    f = ts.f32(inp[:, 0])
    assert (f == np.round(f)).all() and (np.abs(f) <= 1000).all() and (np.abs(f).sum(axis=1) < 2 ** 24).all()
    assert np.array_equal(ts.f32(ts.expected(ts.REDUCE, 0, inp)[:, ts.R_SUM_F32, 0]).astype(np.float64), f.astype(np.float64).sum(axis=1))
    for name, x in ts.reduce_cases().items():
        assert not (x == U32(0x80000000)).any(), "no -0 beside a +0"
        assert (np.isnan(ts.f32(x)).sum(axis=2) <= 2).all()
    assert np.isfinite(ts.f32(ts.reduce_cases()["floats"])).all()


# ---- the cases are what the table says ------------------------------------------------------------------------------------------
def test_path_model_on_the_boundary_cases():
    """class 3: every case the table calls fast is predicted fast, every fallback case fallback; both kinds at every T"""
    inp, paths, names = ts.row_boundary()
    ask = ts.row_unsure(inp[:, 0], inp[:, 2] != 0)
    wrong = [n for n, p, a in zip(names, paths, ask) if (p == "fallback") != bool(a)]
    assert not wrong, wrong[:5]
    assert len(inp) >= 256 and paths.count("fast") >= 100 and paths.count("fallback") >= 100
    for T in ts.BOUNDARY_T:
        for kind, (make, path) in ts.BOUNDARY_KINDS.items():
            assert any(n.startswith("%s@T=%#x+" % (kind, T)) for n in names)
    d2, ids, have = inp[:, 0], inp[:, 1], inp[:, 2] != 0
    for t, name in enumerate(names):  # the run: ids descend as squares ascend; 17 ulps, 1 ulp across a word, or inside one word
        if name.startswith("apart17@") or name.startswith("across1@") or name.startswith("inside@") or name.startswith("equal_roots@"):
            sq = np.sort(d2[t][have[t]].astype(np.int64))
            gaps = np.diff(sq)
            near = int(np.argmin(gaps))
            assert gaps[near] == {"apart17": 17, "across1": 1, "inside": 1, "equal_roots": 1}[name.split("@")[0]], name
            lo, hi = (ids[t][(d2[t] == sq[near + i]) & have[t]][0] for i in (0, 1))
            assert lo > hi, name
            if name.startswith("apart17@"):
                assert (sq[near] >> 4) + 2 == sq[near + 1] >> 4 and sq[near] & 15 == 15 and sq[near + 1] & 15 == 0
            if name.startswith("across1@"):
                assert (sq[near] >> 4) + 1 == sq[near + 1] >> 4
            if name.startswith("inside@"):
                assert sq[near] >> 4 == sq[near + 1] >> 4
    for x in (0, 1 << 4, 0x7FFFF0, 0x800000, 0x3F800000, 0x7F7FFF00):  # zero, denormals, ordinary values, the top binade
        assert any(abs(int(T) * 16 - x) <= 0x100 for T in ts.BOUNDARY_T), hex(x)


def test_both_paths_occur_on_random_rows():
    inp = ts.row_random()
    ask = ts.row_unsure(inp[:, 0], inp[:, 2] != 0)
    print("random rows: %.1f %% of the teams ask for the exact network, %.1f %% of the waves fall back"
          % (100.0 * ask.mean(), 100.0 * ask.reshape(-1, 4).any(axis=1).mean()))
    assert ask.any() and not ask.all()
    assert not ask.reshape(-1, 4).any(axis=1).all(), "some wave stays on the fast path"
    dup = ts.row_duplicates()
    assert ts.row_unsure(dup[:, 0], dup[:, 2] != 0).all()
    sets = ts.neighbour_sets(ts.SORTED_ROW)
    assert not ts.row_unsure(sets["fast"][:, 0], sets["fast"][:, 2] != 0).any() and ts.row_unsure(sets["fallback"][:, 0], sets["fallback"][:, 2] != 0).all()


def test_have_masks_and_their_other_lanes():
    inp = ts.row_have_masks()
    masks = [int(sum(1 << l for l in range(16) if row[l])) for row in inp[:, 2]]
    assert set([0, 0xFFFF] + [1 << l for l in range(16)] + [(1 << n) - 1 for n in range(1, 16)]) <= set(masks)
    holes = [m for m in masks[33:] if m & (m + 1)]  # not a prefix
    assert len(masks) == 233 and len(holes) >= 190
    assert np.isnan(ts.f32(inp[:, 0])[inp[:, 2] == 0]).all() and not np.isnan(ts.f32(inp[:, 0])[inp[:, 2] != 0]).any()


def test_sort_inputs_meet_their_preconditions():
    for op in (ts.CLEAN16, ts.CLEAN16_3):
        for name, inp in ts.sort_cases(op).items():
            for t in range(0, inp.shape[0], 7):
                assert ts.is_bitonic([tuple(int(w) for w in inp[t, :, l]) for l in range(16)]), (ts.OP_NAMES[op], name, t)
    assert not ts.is_bitonic([1, 3, 2, 4] + [5] * 12) and ts.is_bitonic([3, 4, 2, 1] + [0] * 12)
    for op in SORTS:
        d = ts.sort_cases(op)["duplicates"]
        assert all(len(np.unique(d[t, 0])) <= 5 for t in range(d.shape[0])) and any(len(np.unique(d[t, 0])) == 1 for t in range(d.shape[0]))


@pytest.mark.parametrize("nreg", [1, 2, 3, 4])
def test_merge_cases_cover_the_table(nreg):
    inp, names = ts.merge_cases(nreg)
    n = 16 * nreg
    assert len(set(names)) == len(names) == 2 * len(ts.MERGE_FILLS) * len(ts.merge_lengths(nreg)) * len(ts.MERGE_KINDS) * 2
    assert set(ts.merge_lengths(nreg)) >= {0, 1, 15, 16, n - 1, n} and (nreg == 1 or 17 in ts.merge_lengths(nreg))
    lst = ts.key64(inp[:, :nreg], inp[:, nreg:2 * nreg]).reshape(-1, n)
    assert (np.diff(lst.astype(np.float64), axis=1) >= 0).all() and (lst[:, 1:] >= lst[:, :-1]).all(), "sorted, empties last"
    cand_root = ts.root_bits(inp[:, [2 * nreg, 2 * nreg + 2]]).reshape(-1, 32)
    want = ts.spec_merge(inp, nreg)
    skipped = took_all = tied_out = 0
    for t, name in enumerate(names):
        fill, length = int(inp[t, 2 * nreg + 4, 0]), int((lst[t] != ts.EMPTY_KEY).sum())
        assert "fill=%d list=%d " % (fill, length) in name
        real = lst[t, :length] >> np.uint64(32)
        if " below " in name and length and fill:
            assert cand_root[t, :fill].max() < real.min()
            took_all += 1
        if " above " in name and length == n and fill:  # no key of the row gets into any register
            assert cand_root[t, :fill].min() > real.max() and np.array_equal(want[t, :2 * nreg], inp[t, :2 * nreg])
            skipped += 1
        if " tied_last " in name and length == n and "full=1" in name and "left_in=0xffffffff" in name and fill >= 15:
            tied_out += int(want[t, 2 * nreg, 0] == want[t, nreg - 1, 15])  # left_out == the last entry's word: what ROW_TIES reads
    assert skipped >= 10 and took_all >= 10 and tied_out >= 3, (skipped, took_all, tied_out)
    sets = ts.neighbour_sets(ts.MERGE, nreg)
    assert (sets["fill32_taking"][:, 2 * nreg + 4] == 32).all() and (sets["fill0"][:, 2 * nreg + 4] == 0).all()


def test_neighbour_layout():
    cases = ts.row_have_masks()[:5]
    others = ts.neighbour_sets(ts.SORTED_ROW)["fallback"]
    teams, at = ts.beside(cases, others)
    assert teams.shape == (80, 3, 16) and at.shape == (5, 4)
    for c in range(5):
        for p in range(4):
            assert at[c, p] % 4 == p and np.array_equal(teams[at[c, p]], cases[c])
            wave = teams[at[c, p] // 4 * 4:at[c, p] // 4 * 4 + 4]
            assert np.array_equal(np.delete(wave, p, axis=0), others)
    assert np.array_equal(ts.four_copies(cases)[4:8], np.repeat(cases[1:2], 4, axis=0))
    assert ts.TEAM_COUNTS[:5] == (1, 2, 3, 4, 5) and ts.TEAM_COUNTS[5] % 4 == 1 and ts.TEAM_COUNTS[5] > 5


def test_ties_straddle_and_levels_answer_both_ways():
    for nreg in (1, 2, 3, 4):
        inp = ts.row_ties_cases(nreg)
        out = ts.expected(ts.ROW_TIES, nreg, inp)
        tie, edge = out[:, 0].any(axis=1), out[:, 1].any(axis=1)
        assert 0.1 < tie.mean() < 0.9 and edge.any() and (tie & ~edge).any() and not (edge & ~tie).any(), (nreg, tie.mean())
        assert set(int(k) for k in inp[:, nreg + 2, 0]) == set(range(1, 16 * nreg + 1))
        last_tie = (inp[:, nreg + 1, 0] != 0) & (inp[:, nreg, 0] == inp[:, nreg - 1, 15])
        assert (out[last_tie, 1, 15] != 0).any(), "a tie with left_out is seen somewhere"
        k = ts.kth_cases(nreg)
        assert set(int(x) for x in k[:, nreg, 0]) == set(range(1, 16 * nreg + 1))
    s = ts.expected(ts.STRADDLE, 0, ts.straddle_cases())
    assert 0.2 < s.mean() < 0.8 and (ts.f32(ts.straddle_cases()[:, 1]) > 0).all()
    lv = ts.expected(ts.FIRST_LEVEL, 0, ts.first_level_cases())
    level = ts.first_level_cases()[:, 7:8]
    assert (lv <= level).all() and (lv < level).mean() > 0.2 and (lv == level).mean() > 0.2 and len(np.unique(lv)) >= 8
