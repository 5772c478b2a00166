"""What the 16-lane team helpers of the TrueKNN kernels must compute (team_lanes.h, team_walk.h, bigk_keys.h), stated in numpy op
by op for tknnDebugTeamLanes (include/owlknn_debug.h), and the seeded cases the tests run.  Nothing in here is a port of a sorting
network or of a DPP sequence: every op is stated by its outcome.

Layout, as the header's: the input of an op is a uint32 array (teams, WIN, 16) -- word w of lane tl of team t at [t, w, tl] --
and the outcome (teams, WOUT, 16).  Team t is lanes 16 (t & 3) .. + 15 of wave t >> 2; the teams a last wave lacks hold zero
words, which only the wave-wide ops (t_wave_max, t_wave_sum, t_rank, t_bcast) can see.

MERGE's left_out: the helper's row loop is wave-uniform, so a second row made of empty keys only is merged by a team exactly when
ANOTHER team of its wave has more than 16 candidates, and the first row is merged even when nobody has a candidate.  An all-empty
row changes no list; when `full` it can only lower left_out to 0x7f7fffff, the empty key's distance word.  So left_out is
specified, and compared, as min(left_out, 0x7f7fffff) -- what t_row_ties makes of it is the same on both sides, a full list's
last real distance being below 0x7f7fffff.
"""
import numpy as np

SORT16, CLEAN16, SORT16_U32, SORTED_ROW, MERGE, KTH, ROW_TIES, STRADDLE, FIRST_LEVEL, REDUCE, MOVES, SORT16_3, CLEAN16_3 = range(13)
OP_NAMES = ["SORT16", "CLEAN16", "SORT16_U32", "SORTED_ROW", "MERGE", "KTH", "ROW_TIES", "STRADDLE", "FIRST_LEVEL", "REDUCE", "MOVES",
            "SORT16_3", "CLEAN16_3"]
NREG_OPS = (MERGE, KTH, ROW_TIES)
MAX_TEAMS = 1 << 20
EMPTY_WORD = 0x7F7FFFFF
EMPTY_KEY = 0x7F7FFFFF00000000
TOP_WORD = 0x7F7FFFF0  # truncated d2 words from here on are never sure (FLT_MAX, inf, NaN)
QNAN = 0x7FC00000
U32, U64, F32 = np.uint32, np.uint64, np.float32
# REDUCE's and MOVES's out words
R_SUM_U32, R_SUM_F32, R_MIN_F32, R_MAX_F32, R_MIN_U32, R_WAVE_MAX, R_WAVE_SUM_LO, R_WAVE_SUM_HI = range(8)
(M_XOR4, M_SHR1, M_DPP_B1, M_DPP_1B, M_DPP_4E, M_DPP_141, M_DPP_140, M_DPP_128, M_DPP_121, M_LANE_READ, M_RANK, M_COUNT, M_COUNT_KEEP,
 M_TEAM_ANY, M_BCAST) = range(15)


def variants(op):
    return (1, 2, 3, 4) if op in NREG_OPS else (0,)


def words(op, variant=0):
    """(WIN, WOUT) of an op: the header's table."""
    n = variant
    return {SORT16: (2, 2), CLEAN16: (2, 2), SORT16_U32: (1, 1), SORTED_ROW: (3, 2), MERGE: (2 * n + 7, 2 * n + 1), KTH: (n + 1, 1),
            ROW_TIES: (n + 10, 2), STRADDLE: (5, 1), FIRST_LEVEL: (8, 1), REDUCE: (1, 8), MOVES: (4, 15), SORT16_3: (3, 3),
            CLEAN16_3: (3, 3)}[op]


def f32(bits):
    return np.ascontiguousarray(bits, U32).view(F32)


def bits(x):
    return np.ascontiguousarray(x, F32).view(U32)


def key64(hi, lo):
    return (np.asarray(hi, U64) << U64(32)) | np.asarray(lo, U64)


def root_bits(d2_bits):
    """bits of the IEEE float32 square root of the float32 with these bits (numpy's float32 sqrt is correctly rounded)"""
    with np.errstate(invalid="ignore"):
        return bits(np.sqrt(f32(d2_bits)))


def _split(keys):
    return (keys >> U64(32)).astype(U32), (keys & U64(0xFFFFFFFF)).astype(U32)


# ---- the ops ------------------------------------------------------------------------------------------------------------------
def spec_sort16(inp):
    kd, ki = _split(np.sort(key64(inp[:, 0], inp[:, 1]), axis=1))
    return np.stack([kd, ki], axis=1)


def spec_sort16_u32(inp):
    return np.sort(inp, axis=2)


def spec_sort16_3(inp):
    order = np.argsort(inp[:, 2], axis=1, kind="stable")
    for w in (1, 0):
        order = np.take_along_axis(order, np.argsort(np.take_along_axis(inp[:, w], order, axis=1), axis=1, kind="stable"), axis=1)
    return np.stack([np.take_along_axis(inp[:, w], order, axis=1) for w in range(3)], axis=1)


def row_keys(d2_bits, ids, have):
    """the sorted row t_sorted_row owes: the lanes with `have` as (root, id) keys in uint64 order, KNN_EMPTY_KEY for the others"""
    keys = np.where(np.asarray(have, bool), key64(root_bits(d2_bits), ids), U64(EMPTY_KEY))
    return np.sort(keys, axis=-1)


def spec_sorted_row(inp):
    kd, ki = _split(row_keys(inp[:, 0], inp[:, 1], inp[:, 2] != 0))
    return np.stack([kd, ki], axis=1)


def row_unsure(d2_bits, have):
    """The model of t_sorted_row's path decision, per team: True where some lane is `unsure`, i.e. the team asks for the exact
    network.  (The decision itself is one ballot over a wave: a wave falls back if any of its teams asks.)  Only the tests of
    which path a case takes read this; no expected key depends on it."""
    lanes = np.arange(16, dtype=U32)
    w = np.where(np.asarray(have, bool), (np.asarray(d2_bits, U32) & U32(0xFFFFFFF0)) | lanes, U32(0xFFFFFFF0) | lanes)
    w = np.sort(w, axis=-1)
    real = w < U32(0xFFFFFFF0)
    close = np.zeros(w.shape, bool)
    close[..., 1:] = ((w[..., 1:] >> U32(4)) - (w[..., :-1] >> U32(4))) <= U32(1)
    return (real & (close | (w >= U32(TOP_WORD)))).any(axis=-1)


def spec_merge(inp, nreg):
    t = inp.shape[0]
    out = np.zeros((t, 2 * nreg + 1, 16), U32)
    lst = key64(inp[:, :nreg], inp[:, nreg:2 * nreg]).reshape(t, 16 * nreg)  # entry 16 j + tl
    cand = key64(root_bits(inp[:, [2 * nreg, 2 * nreg + 2]]), inp[:, [2 * nreg + 1, 2 * nreg + 3]]).reshape(t, 32)
    for i in range(t):
        fill, left, full = int(inp[i, 2 * nreg + 4, 0]), int(inp[i, 2 * nreg + 5, 0]), bool(inp[i, 2 * nreg + 6, 0])
        both = np.sort(np.concatenate([lst[i], cand[i, :fill]]))
        keep, leave = both[:16 * nreg], both[16 * nreg:]
        if full and len(leave):
            left = min(left, int(leave[0] >> U64(32)))
        kd, ki = _split(keep)
        out[i, :nreg], out[i, nreg:2 * nreg] = kd.reshape(nreg, 16), ki.reshape(nreg, 16)
        out[i, 2 * nreg] = min(left, EMPTY_WORD)
    return out


def clamp_left_out(out, nreg):
    """the comparison form of a MERGE outcome: left_out as min(left_out, 0x7f7fffff) (module docstring)"""
    out = out.copy()
    out[:, 2 * nreg] = np.minimum(out[:, 2 * nreg], U32(EMPTY_WORD))
    return out


def spec_kth(inp, nreg):
    t = inp.shape[0]
    k = inp[:, nreg].astype(np.int64)  # per lane: each reads its own copy
    lst = inp[:, :nreg].reshape(t, 16 * nreg)
    return np.take_along_axis(lst, k - 1, axis=1)[:, None, :]


def straddle(d, r0, r_last, qmax, span):
    """tie_may_straddle in float32, every operation rounded on its own; needs r0 > 0"""
    d, r0, r_last, qmax, span = np.broadcast_arrays(*[np.asarray(x, F32) for x in (d, r0, r_last, qmax, span)])
    assert (r0 > 0).all()
    res = np.zeros(d.shape, bool)
    todo = np.ones(d.shape, bool)
    r = r0.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        while todo.any():
            mg = (qmax + F32(2.0) * r) * F32(4.76837158203125e-07)
            no = todo & (d <= (r - mg) * F32(0.99999))
            todo &= ~no
            yes = todo & ((d <= (r + mg) * span) | ~(r < r_last))
            res |= yes
            todo &= ~yes
            r = r * F32(2.0)
    return res


def spec_straddle(inp):
    x = f32(inp)
    return straddle(x[:, 0], x[:, 1], x[:, 2], x[:, 3], x[:, 4]).astype(U32)[:, None, :]


def spec_row_ties(inp, nreg):
    """KList::has_ties per entry: entry j in 1 .. k ties if its distance word is entry j - 1's; the last entry of the registers
    also if `full` and left_out is its word; each tie counts only where `look` holds and tie_may_straddle says the two may have
    become candidates in different rounds; `edge`: the tie is with a candidate that is not written (entry k, or the one left out)."""
    t = inp.shape[0]
    n = 16 * nreg
    e = inp[:, :nreg].reshape(t, n)
    per_lane = lambda w: np.tile(inp[:, w], (1, nreg))  # noqa: E731  the word of the lane that holds entry j
    left, full, k, look = per_lane(nreg), per_lane(nreg + 1) != 0, per_lane(nreg + 2).astype(np.int64), per_lane(nreg + 9) != 0
    q = np.abs(np.stack([f32(per_lane(nreg + 3 + a)) for a in range(3)]))
    qmax = np.maximum(np.maximum(q[0], q[1]), q[2])
    r0, r, span = f32(per_lane(nreg + 6)), f32(per_lane(nreg + 7)), f32(per_lane(nreg + 8))
    j = np.arange(n)[None, :]
    tie = np.zeros((t, n), bool)
    tie[:, 1:] = e[:, 1:] == e[:, :-1]
    tie &= j <= k
    out_t = (j == n - 1) & full & (left == e)
    tie |= out_t
    tie &= look & straddle(f32(e), r0, r, qmax, span)
    edge = tie & ((j == k) | out_t)
    return np.stack([tie.reshape(t, nreg, 16).any(axis=1), edge.reshape(t, nreg, 16).any(axis=1)], axis=1).astype(U32)


def in_box(c, r, q):
    """knn_in_box: fl32(c - r) <= q <= fl32(c + r) on all three axes (oracle/trueknn_numpy.py states the same test)"""
    r = np.asarray(r, F32)[None]
    with np.errstate(over="ignore", invalid="ignore"):
        return (((c - r).astype(F32) <= q) & (q <= (c + r).astype(F32))).all(axis=0)


def spec_first_level(inp):
    x = f32(inp)
    p, q = np.stack([x[:, 0], x[:, 1], x[:, 2]]), np.stack([x[:, 3], x[:, 4], x[:, 5]])
    level = np.clip(inp[:, 7].view(np.int32), 0, 64)
    rr = x[:, 6].copy()
    res = level.copy()
    found = np.zeros(level.shape, bool)
    with np.errstate(over="ignore"):
        for lvl in range(64):
            hit = ~found & (lvl < level) & in_box(p, rr, q)
            res[hit] = lvl
            found |= hit
            rr = rr * F32(2.0)
    return res.astype(U32)[:, None, :]


def _waves(a):
    """(teams, 16) -> (waves, 64), the missing teams of the last wave as zero words"""
    t = a.shape[0]
    full = np.zeros(((t + 3) // 4 * 4, 16), a.dtype)
    full[:t] = a
    return full.reshape(-1, 64)


def spec_reduce(inp):
    """Out word R_SUM_F32 is given as the float32 nearest the float64 sum: the helper owes it only within fsum_bound()."""
    v = inp[:, 0]
    t = v.shape[0]
    f = f32(v)
    out = np.zeros((t, 8, 16), U32)
    rep = lambda x: np.repeat(np.asarray(x)[:, None], 16, axis=1)  # noqa: E731
    out[:, R_SUM_U32] = rep(v.astype(U64).sum(axis=1).astype(U32))
    with np.errstate(over="ignore", invalid="ignore"):
        out[:, R_SUM_F32] = rep(bits(f.astype(np.float64).sum(axis=1).astype(F32)))
    out[:, R_MIN_F32] = rep(bits(np.fmin.reduce(f, axis=1)))
    out[:, R_MAX_F32] = rep(bits(np.fmax.reduce(f, axis=1)))
    out[:, R_MIN_U32] = rep(v.min(axis=1))
    wmax = bits(np.fmax.reduce(f32(_waves(v)), axis=1))
    wsum = _waves(v).astype(U64).sum(axis=1)
    team_wave = np.arange(t) // 4
    out[:, R_WAVE_MAX] = rep(wmax[team_wave])
    out[:, R_WAVE_SUM_LO] = rep((wsum & U64(0xFFFFFFFF)).astype(U32)[team_wave])
    out[:, R_WAVE_SUM_HI] = rep((wsum >> U64(32)).astype(U32)[team_wave])
    return out


def fsum_bound(inp):
    """(float64 sum, bound) per team for t_team_sum(float): four rounded additions per lane, each on a partial sum no larger than
    the sum of the magnitudes: |lane 0's value - sum| <= 4 * 2^-24 * sum |x|"""
    f = f32(inp[:, 0]).astype(np.float64)
    return f.sum(axis=1), 4.0 * 2.0 ** -24 * np.abs(f).sum(axis=1)


def spec_moves(inp, variant):
    v, src, bit, acc = inp[:, 0], inp[:, 1] & U32(15), (inp[:, 2] != 0), inp[:, 3]
    t = v.shape[0]
    lanes = np.arange(16)
    out = np.zeros((t, 15, 16), U32)
    out[:, M_XOR4] = v[:, lanes ^ 4]
    out[:, M_SHR1, 1:] = v[:, :-1]
    for word, x in ((M_DPP_B1, 1), (M_DPP_1B, 3), (M_DPP_4E, 2), (M_DPP_141, 7), (M_DPP_140, 15), (M_DPP_128, 8)):
        out[:, word] = v[:, lanes ^ x]
    out[:, M_DPP_121] = v[:, (lanes - 1) % 16]
    out[:, M_LANE_READ] = np.take_along_axis(v, src.astype(np.int64), axis=1)
    wave_bits = _waves(bit.astype(np.int64))
    below = (np.cumsum(wave_bits, axis=1) - wave_bits).reshape(-1, 16)[:t]  # set bits of the wave's mask below my lane
    out[:, M_RANK] = below.astype(U32)
    out[:, M_COUNT] = (acc.astype(U64) + bit).astype(U32)
    out[:, M_COUNT_KEEP] = out[:, M_COUNT]
    out[:, M_TEAM_ANY] = np.repeat(bit.any(axis=1)[:, None], 16, axis=1)
    out[:, M_BCAST] = np.repeat(_waves(v)[np.arange(t) // 4, variant][:, None], 16, axis=1)
    return out


def expected(op, variant, inp):
    inp = np.ascontiguousarray(inp, U32)
    assert inp.shape[1:] == (words(op, variant)[0], 16), (OP_NAMES[op], inp.shape)
    if op in (SORT16, CLEAN16):
        return spec_sort16(inp)
    if op == SORT16_U32:
        return spec_sort16_u32(inp)
    if op in (SORT16_3, CLEAN16_3):
        return spec_sort16_3(inp)
    if op == SORTED_ROW:
        return spec_sorted_row(inp)
    if op == MERGE:
        return spec_merge(inp, variant)
    if op == KTH:
        return spec_kth(inp, variant)
    if op == ROW_TIES:
        return spec_row_ties(inp, variant)
    if op == STRADDLE:
        return spec_straddle(inp)
    if op == FIRST_LEVEL:
        return spec_first_level(inp)
    if op == REDUCE:
        return spec_reduce(inp)
    assert op == MOVES
    return spec_moves(inp, variant)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _rng(*seed):
    return np.random.default_rng([20240611, *seed])


def rand_u32(rng, shape):
    return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(U32)


def rand_d2(rng, shape, specials=True):
    """bits of squared distances over every binade, the denormals among them; with `specials` a few 0, FLT_MAX and +inf"""
    b = (rng.integers(0, 255, size=shape, dtype=np.uint64) << np.uint64(23)) | rng.integers(0, 1 << 23, size=shape, dtype=np.uint64)
    b = b.astype(U32)
    if specials:
        pick = rng.random(shape)
        b = np.where(pick < 0.01, U32(0), np.where(pick < 0.02, U32(0x7F7FFFFF), np.where(pick < 0.03, U32(0x7F800000), b)))
    return b


def _dup_words(rng, teams, pool_of):
    """(teams, 16) words, team t drawing from 1, 2, 3 or 5 distinct ones of pool_of(rng, 5)"""
    out = np.zeros((teams, 16), U32)
    for t in range(teams):
        pool = pool_of(rng, 5)[:(1, 2, 3, 5)[t % 4]]
        out[t] = pool[rng.integers(0, len(pool), 16)]
    return out


def _bitonic(rng, inp):
    """the teams' keys rearranged along the lanes into a bitonic sequence: some ascending, the others descending, rotated"""
    nw = inp.shape[1]
    out = spec_sort16_3(inp) if nw == 3 else (spec_sort16(inp) if nw == 2 else spec_sort16_u32(inp))
    for t in range(out.shape[0]):
        up = rng.random(16) < rng.random()
        order = np.concatenate([np.nonzero(up)[0], np.nonzero(~up)[0][::-1]])
        out[t] = np.roll(out[t][:, order], int(rng.integers(0, 16)), axis=1)
    return out


def sort_cases(op, teams=512):
    """{class: input} of SORT16, CLEAN16, SORT16_U32, SORT16_3, CLEAN16_3"""
    nw = {SORT16: 2, CLEAN16: 2, SORT16_U32: 1, SORT16_3: 3, CLEAN16_3: 3}[op]
    rng = _rng(1, op)
    random = rand_u32(rng, (teams, nw, 16))
    dups = rand_u32(rng, (teams, nw, 16))
    for w in range(nw - 1 if nw > 1 else 1):  # all words but the last from a few values: the last word decides
        dups[:, w] = _dup_words(rng, teams, lambda g, n: rand_u32(g, n))
    if nw > 1:
        dups[::3, nw - 1] &= U32(3)  # and wholly equal keys
    cases = {"random": random, "duplicates": dups}
    if op == SORT16_U32:  # the words t_sorted_row sorts: truncated squares with the lane in their last four bits
        cases["truncated"] = ((rand_d2(rng, (teams, 1, 16)) & U32(0xFFFFFFF0)) | np.arange(16, dtype=U32))
        cases["truncated"][::2, 0, :] = (_dup_words(rng, teams // 2, lambda g, n: rand_d2(g, n)) & U32(0xFFFFFFF0)) | np.arange(16, dtype=U32)
    if op in (CLEAN16, CLEAN16_3):
        cases = {name: _bitonic(rng, x) for name, x in cases.items()}
    return cases


def is_bitonic(keys):
    """keys: a sequence of comparable items along the lanes -- ascending then descending, or a rotation of that"""
    n = len(keys)
    for rot in range(n):
        s = [keys[(rot + i) % n] for i in range(n)]
        i = 0
        while i + 1 < n and s[i] <= s[i + 1]:
            i += 1
        while i + 1 < n and s[i] >= s[i + 1]:
            i += 1
        if i == n - 1:
            return True
    return False


def _row_input(d2, ids, have):
    return np.stack([np.asarray(d2, U32), np.asarray(ids, U32), np.asarray(have).astype(U32)], axis=1)


def row_random(teams=1024):
    rng = _rng(2)
    return _row_input(rand_d2(rng, (teams, 16)), rand_u32(rng, (teams, 16)), np.ones((teams, 16), bool))


def row_duplicates(teams=512):
    rng = _rng(3)
    return _row_input(_dup_words(rng, teams, lambda g, n: rand_d2(g, n, specials=False)), rand_u32(rng, (teams, 16)), np.ones((teams, 16), bool))


BOUNDARY_T = [0, 1, 2, 1000, 0x7FFFD, 0x7FFFE, 0x7FFFF, 0x80000, 0x3F80000, 0x3F80001, 0x3FFFFFE, 0x4000000, 0x4123456, 0x7F00000,
              (TOP_WORD >> 4) - 9, (TOP_WORD >> 4) - 7]  # zero, denormals, their end, ordinary values, the top binade
# the squares of a case around truncated word T, ascending, and the path the case must take.  17 ulps: the nearest pair that
# stays on the fast path; across one word boundary or inside one word: the exact network
BOUNDARY_KINDS = {
    "apart17": (lambda T: [T * 16 + 15, (T + 2) * 16], "fast"),
    "apart17_run3": (lambda T: [T * 16 + 15, (T + 2) * 16, (T + 4) * 16], "fast"),
    "apart17_run4": (lambda T: [T * 16 + 15, (T + 2) * 16, (T + 4) * 16, (T + 6) * 16], "fast"),
    "across1": (lambda T: [T * 16 + 15, (T + 1) * 16], "fallback"),
    "across1_run3": (lambda T: [T * 16 + 15, (T + 1) * 16, (T + 1) * 16 + 15], "fallback"),
    "across1_run4": (lambda T: [T * 16 + 15, (T + 1) * 16, (T + 1) * 16 + 15, (T + 2) * 16], "fallback"),
    "inside": (lambda T: [T * 16 + 3, T * 16 + 4], "fallback"),
    "inside_run3": (lambda T: [T * 16, T * 16 + 1, T * 16 + 2], "fallback"),
    "inside_run4": (lambda T: [T * 16 + 12, T * 16 + 13, T * 16 + 14, T * 16 + 15], "fallback"),
    "equal": (lambda T: [T * 16 + 7, T * 16 + 7, T * 16 + 7], "fallback"),
}


def equal_root_pairs(count=24):
    """squares x, x + 1 (as bits) whose rounded roots coincide, over the binades: `count` inside one truncated word and as many
    across a word boundary (x ends in 15) -- the pairs one word apart that the fast path would order by their lanes"""
    rng = _rng(4)
    found = [[], []]
    while min(len(f) for f in found) < count:
        x = rand_d2(rng, 64, specials=False)
        for across in (0, 1):
            y = (x | U32(15)) if across else x[(x & U32(15)) != 15]
            y = y[(y > 16) & (y < TOP_WORD - 16)]
            found[across] += [int(v) for v in y[root_bits(y) == root_bits(y + U32(1))]]
    return found[0][:count] + found[1][:count]


def row_boundary():
    """(input, the path each team must take by the table, a name per team).  Every case three times: the run alone, with three and
    with eleven other squares far from it and from each other; the run's ids descend as its squares ascend, on random lanes."""
    rng = _rng(5)
    runs = [(name + "@T=%#x" % T, make(T), path) for name, (make, path) in BOUNDARY_KINDS.items() for T in BOUNDARY_T]
    runs += [("equal_roots@%#x" % x, [x, x + 1], "fallback") for x in equal_root_pairs()]
    runs += [("top@%#x" % x, [x], "fallback") for x in (TOP_WORD, 0x7F7FFFFF, 0x7F800000)]
    d2, ids, have, paths, names = [], [], [], [], []
    for name, run, path in runs:
        T = run[0] >> 4
        for others in (0, 3, 11):
            step = 1 if T < (1 << 26) else -1
            far = [(T + step * (100 + 10 * i)) * 16 + int(rng.integers(0, 16)) for i in range(others)]
            vals = run + far
            lanes = rng.permutation(16)[:len(vals)]
            row_d2, row_id, row_have = np.full(16, QNAN, U32), rand_u32(rng, 16), np.zeros(16, bool)
            row_d2[lanes], row_have[lanes] = np.array(vals, U32), True
            top = int(rng.integers(100, 1 << 31))
            row_id[lanes[:len(run)]] = top - np.arange(len(run))  # the larger id on the smaller square
            d2.append(row_d2), ids.append(row_id), have.append(row_have), paths.append(path), names.append("%s+%d" % (name, others))
    return _row_input(np.array(d2), np.array(ids), np.array(have)), paths, names


def row_have_masks():
    """empty, full, every single lane, every prefix, 200 random masks with holes; lanes without `have` carry NaN squares and any id"""
    rng = _rng(6)
    masks = [0, 0xFFFF] + [1 << l for l in range(16)] + [(1 << n) - 1 for n in range(1, 16)] + [int(m) for m in rng.integers(1, 0xFFFF, 200)]
    have = np.array([[(m >> l) & 1 for l in range(16)] for m in masks], bool)
    d2 = rand_d2(rng, have.shape)
    nan = np.where(rng.random(have.shape) < 0.5, U32(QNAN), U32(0x7F800000) + rng.integers(1, 1 << 23, have.shape).astype(U32))
    return _row_input(np.where(have, d2, nan), rand_u32(rng, have.shape), have)


MERGE_FILLS = (0, 1, 15, 16, 17, 31, 32)
MERGE_KINDS = ("below", "above", "interleaved", "tied_last", "duplicates")


def merge_lengths(nreg):
    return sorted({0, 1, 15, 16, 17, 16 * nreg - 1, 16 * nreg} & set(range(16 * nreg + 1)))


def _squares_in(rng, lo, hi, n):
    return bits(rng.uniform(lo, hi, n).astype(F32))


def merge_cases(nreg):
    """(input, a name per team): every `full`, fill, list length, kind of candidates and left_out of the case table.  The list's
    roots lie in [1, 2); candidates below it, above it (no key of the row gets into any register), among it, at the root of its
    last entry with ids on both sides of that entry's, or from three squares only."""
    rng = _rng(7, nreg)
    n = 16 * nreg
    rows, names = [], []
    for full in (0, 1):
        for fill in MERGE_FILLS:
            for length in merge_lengths(nreg):
                for kind in MERGE_KINDS:
                    for left in (0xFFFFFFFF, 0):
                        lst = np.sort(key64(root_bits(_squares_in(rng, 1.0, 4.0, length)), rand_u32(rng, length) >> U32(1)))
                        lst = np.concatenate([lst, np.full(n - length, EMPTY_KEY, U64)])
                        if kind == "below":
                            c_d2 = _squares_in(rng, 0.01, 0.5, 32)
                        elif kind in ("above", "tied_last"):  # (tied_last: the other candidates stay out, the ties compete)
                            c_d2 = _squares_in(rng, 8.0, 16.0, 32)
                        elif kind == "duplicates":
                            c_d2 = _squares_in(rng, 1.0, 4.0, 3)[rng.integers(0, 3, 32)]
                        else:
                            c_d2 = _squares_in(rng, 1.0, 4.0, 32)
                        c_id = rand_u32(rng, 32) >> U32(1)
                        if kind == "tied_last" and length:
                            last_d, last_i = int(lst[length - 1] >> U64(32)), int(lst[length - 1] & U64(0xFFFFFFFF))
                            root = f32(np.array([last_d], U32))
                            square = bits(root * root)[0]
                            assert root_bits(np.array([square], U32))[0] == last_d
                            tied = rng.random(32) < 0.5
                            c_d2 = np.where(tied, square, c_d2)
                            c_id = np.where(tied, np.where(rng.random(32) < 0.5, U32(last_i // 2), U32(min(last_i + 7, 0xFFFFFFFF))), c_id)
                        kd, ki = _split(lst)
                        one = [kd.reshape(nreg, 16), ki.reshape(nreg, 16), c_d2.reshape(2, 16)[:1], c_id.reshape(2, 16)[:1], c_d2.reshape(2, 16)[1:],
                               c_id.reshape(2, 16)[1:]] + [np.full((1, 16), x, U32) for x in (fill, left, full)]
                        rows.append(np.concatenate(one).astype(U32))
                        names.append("full=%d fill=%d list=%d %s left_in=%#x" % (full, fill, length, kind, left))
    return np.array(rows, U32), names


def neighbour_sets(op, variant=0):
    """Two sets of three teams a case of classes 3 to 5 is put beside: for SORTED_ROW three that stay on the fast path and three
    that ask for the exact network; for MERGE three with fill = 32 that take keys into every register and three with fill = 0."""
    if op == SORTED_ROW:
        pool = row_random(256)
        ask = row_unsure(pool[:, 0], pool[:, 2] != 0)
        dup = row_duplicates(4)
        assert (~ask).sum() >= 3 and row_unsure(dup[:, 0], dup[:, 2] != 0).all()
        return {"fast": pool[~ask][:3], "fallback": dup[:3]}
    assert op == MERGE
    x, names = merge_cases(variant)
    taking = [i for i, s in enumerate(names) if s.startswith("full=1 fill=32 list=%d below" % (16 * variant))][:3]
    idle = [i for i, s in enumerate(names) if s.startswith("full=0 fill=0 list=%d above" % (16 * variant))][:3]
    idle = (idle * 3)[:3]
    taking = (taking * 3)[:3]
    return {"fill32_taking": x[taking], "fill0": x[idle]}


def beside(cases, others):
    """Every case in each of the four team positions of a wave beside the three teams `others`: (teams, where each case sits).
    Case c at position p is team 4 * (4 * c + p) + p."""
    c, shape = cases.shape[0], cases.shape[1:]
    waves = np.zeros((c, 4, 4) + shape, U32)
    at = np.zeros((c, 4), np.int64)
    for p in range(4):
        waves[:, p, [s for s in range(4) if s != p]] = others[None]
        waves[:, p, p] = cases
        at[:, p] = 4 * (4 * np.arange(c) + p) + p
    return waves.reshape((c * 16,) + shape), at


def four_copies(cases):
    """every case as the four teams of a wave of its own"""
    return np.repeat(cases, 4, axis=0)


def kth_cases(nreg, teams=256):
    rng = _rng(8, nreg)
    k = np.repeat(rng.integers(1, 16 * nreg + 1, (teams, 1, 1)), 16, axis=2).astype(U32)
    k[:16 * nreg, 0, :] = np.arange(1, 16 * nreg + 1, dtype=U32)[:, None]  # every k once
    return np.concatenate([rand_u32(rng, (teams, nreg, 16)), k], axis=1)


def row_ties_cases(nreg, teams=1024):
    """Lists of a few distinct distances around the radii r0 2^l (so that tie_may_straddle answers both ways), with empties, every
    k, full or not, left_out at the last entry's word, above it and unset, look on and off, both spans."""
    rng = _rng(9, nreg)
    n = 16 * nreg
    inp = np.zeros((teams, nreg + 10, 16), U32)
    for t in range(teams):
        r0 = F32(rng.uniform(0.01, 1.0))
        level = int(rng.integers(0, 6))
        r = F32(r0 * F32(2.0 ** level))
        factors = np.array([0.0, 0.3, 0.5773, 0.58, 0.7, 0.99, 0.999995, 1.0, 1.00001, 1.2, 1.7, 1.74], F32)
        pool = np.sort(bits((F32(r0) * F32(2.0) ** rng.integers(0, level + 1, 6).astype(F32)) * factors[rng.integers(0, len(factors), 6)]))
        length = int(rng.integers(0, n + 1)) if t % 3 else n
        e = np.concatenate([np.sort(pool[rng.integers(0, rng.integers(1, 7), length)]), np.full(n - length, EMPTY_WORD, U32)])
        k = int(rng.integers(1, n + 1)) if t >= n else t + 1
        left = (int(e[n - 1]), int(e[n - 1]) + 1, 0xFFFFFFFF)[t % 3 if t % 2 else 0]
        q = bits(rng.uniform(-100.0, 100.0, 3).astype(F32))
        span = bits(np.array([(1.73206, 1.41422)[t % 2]], F32))[0]
        scal = [left, int(rng.random() < 0.7), k, q[0], q[1], q[2], int(bits(r0)[0]), int(bits(r)[0]), span, int(rng.random() < 0.85)]
        inp[t, :nreg] = e.reshape(nreg, 16)
        inp[t, nreg:] = np.array(scal, U32)[:, None]
    return inp


def straddle_cases(teams=512):
    rng = _rng(10)
    shape = (teams, 16)
    r0 = rng.uniform(0.001, 10.0, shape).astype(F32)
    last = rng.integers(0, 9, shape)
    r_last = r0 * (F32(2.0) ** last.astype(F32))
    at = r0 * (F32(2.0) ** rng.integers(0, 9, shape).astype(F32))  # a radius of the sequence, also beyond the last one
    factors = np.array([0.0, 0.25, 0.57, 0.5773503, 0.578, 0.9, 0.99998, 0.99999, 1.0, 1.000001, 1.41, 1.415, 1.73, 1.7321, 5.0], F32)
    d = at * factors[rng.integers(0, len(factors), shape)]
    d = np.clip(bits(d).astype(np.int64) + rng.integers(-2, 3, shape), 0, 0x7F7FFFFF).astype(U32)
    qmax = np.where(rng.random(shape) < 0.3, F32(0), rng.uniform(0.0, 1000.0, shape).astype(F32))
    span = np.where(rng.random(shape) < 0.5, F32(1.73206), F32(1.41422))
    return np.stack([d, bits(r0), bits(r_last), bits(qmax), bits(span)], axis=1)


def first_level_cases(teams=512):
    """points whose Chebyshev distance from the query is a radius of the doubling sequence, give or take a few ulps, on one axis"""
    rng = _rng(11)
    shape = (teams, 16)
    q = rng.uniform(-50.0, 50.0, (3,) + shape).astype(F32)
    r0 = rng.uniform(0.01, 2.0, shape).astype(F32)
    level = rng.integers(0, 9, shape)
    at = r0 * (F32(2.0) ** rng.integers(0, 10, shape).astype(F32))
    off = (at[None] * rng.uniform(-1.0, 1.0, (3,) + shape).astype(F32)).astype(F32)
    axis = rng.integers(0, 3, shape)
    sign = np.where(rng.random(shape) < 0.5, F32(-1), F32(1))
    for a in range(3):
        off[a] = np.where(axis == a, sign * at, off[a])
    p = (q + off).astype(F32)
    nudge = rng.integers(-2, 3, shape)
    for a in range(3):
        p[a] = np.where(axis == a, f32((bits(p[a]).astype(np.int64) + nudge).astype(U32)), p[a])
    return np.stack([bits(p[0]), bits(p[1]), bits(p[2]), bits(q[0]), bits(q[1]), bits(q[2]), bits(r0), level.astype(U32)], axis=1)


def reduce_cases(teams=512):
    """{class: input}.  `words`: any bits with the NaNs and -0 taken out and one quiet NaN in some teams (fminf ignores it; +0 and
    -0 are not mixed); `floats`: finite values of moderate size for the sum's bound; `small_integers`: every order of addition is
    exact, so all sixteen lanes owe the same word."""
    rng = _rng(12)
    w = rand_d2(rng, (teams, 1, 16)) | (rand_u32(rng, (teams, 1, 16)) & U32(0x80000000))
    w = np.where(w == U32(0x80000000), U32(0), w)
    w[::5, 0, 3] = QNAN
    w[::7, 0, 11] = QNAN
    floats = bits((rng.uniform(-1.0, 1.0, (teams, 1, 16)) * 2.0 ** rng.integers(-20, 21, (teams, 1, 16))).astype(F32))
    ints = bits(rng.integers(-1000, 1001, (teams, 1, 16)).astype(F32))
    ints = np.where(ints == U32(0x80000000), U32(0), ints)
    return {"words": w, "floats": floats, "small_integers": ints}


MOVES_BCAST_LANES = (0, 17, 38, 63)


def moves_cases(teams=256):
    rng = _rng(13)
    bit = rng.random((teams, 16)) < rng.random((teams, 1))
    bit[::9] = False
    bit[4::9] = True
    acc = rand_u32(rng, (teams, 16))
    acc[::4, 0] = 0xFFFFFFFF  # the carry out of the add
    return np.stack([rand_u32(rng, (teams, 16)), rng.integers(0, 16, (teams, 16)).astype(U32), bit.astype(U32), acc], axis=1)


def random_cases(op, variant=0):
    """the random class of an op (class 7 runs its first 1, 2, 3, 4, 5 and 4 N + 1 teams)"""
    if op in (SORT16, CLEAN16, SORT16_U32, SORT16_3, CLEAN16_3):
        return sort_cases(op)["random"]
    return {SORTED_ROW: row_random, MERGE: lambda: merge_cases(variant)[0], KTH: lambda: kth_cases(variant), ROW_TIES: lambda: row_ties_cases(variant),
            STRADDLE: straddle_cases, FIRST_LEVEL: first_level_cases, REDUCE: lambda: reduce_cases()["words"], MOVES: moves_cases}[op]()


TEAM_COUNTS = (1, 2, 3, 4, 5, 4 * 33 + 1)
