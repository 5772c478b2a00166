"""What the device side of the sharded driver must return, restated in numpy, and the cases its tests share: tknnHaloSelect and
tknnHaloSelectFixed (which of a tile's points go to which peer), tknnSegmentMin (the smallest value of every segment) and the sets
tknnDbscanAssign is run on.  No tests here, and nothing the library reads.

  * select: peer p receives the rows of P inside the CLOSED float32 box of any of p's boxes, each once however many of p's boxes
    hold it.  Plain numpy comparisons: a NaN coordinate is inside nothing, a box with lo > hi or a NaN bound holds nothing.  A
    row is `boundary` if some box of some peer holds it.
  * segment_min: out[s] = min(out[s], value[i]) over the entries with segment[i] == s >= 0, in int64 (np.minimum.at).
  * the expected labels of tknnDbscanAssign are dbscan_query_spec.query_labels' (brute force) for the rows that are not core.

The cases are named generators with fixed seeds; every one has at most 20 000 points.  tests/test_halo_expectations.py shows on
the CPU that they are what they claim to be.
"""
import numpy as np

import oracle
from owlraytracing_amd import datasets
from owlraytracing_amd.datasets import pad_to_3d

import dbscan_query_spec as dq

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
FLT_MAX = np.finfo(np.float32).max


# ---- selection ------------------------------------------------------------------------------------------------------------------

def inside_boxes(P, boxes):
    """(nboxes, n) bool: row i of P inside the closed box j."""
    P = pad_to_3d(np.asarray(P, np.float32))
    boxes = np.asarray(boxes, np.float32).reshape(-1, 6)
    with np.errstate(invalid="ignore"):
        return np.all((P[None, :, :] >= boxes[:, None, :3]) & (P[None, :, :] <= boxes[:, None, 3:]), axis=2)


def select(P, ids, boxes, box_peer, npeers):
    """(lists, boundary): lists[p] the sorted ids of the rows of P inside any box of peer p, boundary (n,) bool "inside some box of
    some peer"."""
    ids = np.asarray(ids)
    box_peer = np.asarray(box_peer, np.int64).reshape(-1)
    hit = inside_boxes(P, boxes)
    assert hit.shape == (len(box_peer), len(ids))
    lists, boundary = [], np.zeros(len(ids), bool)
    for p in range(npeers):
        mine = hit[box_peer == p].any(axis=0) if len(box_peer) else np.zeros(len(ids), bool)
        lists.append(np.sort(ids[mine]))
        boundary |= mine
    return lists, boundary


# the leaf-block border (16 points), the workgroup border of the point kernel (256 points) and that of the block-mask kernel
# (256 leaf blocks = 4 096 points), and an irregular size
SELECT_N = (1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 19_997)
FIXED_N = (17, 257, 4097, 19_997)
FAMILIES = ("scattered", "peers_apart", "peers_all", "everything_max", "everything_inf", "overlaps", "degenerate", "no_boxes",
            "one_peer", "planar")
FIXED_FAMILIES = ("scattered", "peers_apart", "peers_all", "overlaps")
PEERS_APART = (0, 1, 31, 32, 33, 62, 63)

_points = {}


def points(n, planar=False):
    """(P (n,3) float32, ids (n,) int32, nan_rows): uniform points, ids a non-monotone map far outside 0..n-1, and -- from n = 15
    up -- a few rows with a NaN in one coordinate.  Cached; do not write to them."""
    key = (n, planar)
    if key not in _points:
        rng = np.random.default_rng(7000 + n)
        P = datasets.uniform3d(n, seed=700 + n).astype(np.float32)
        if planar:
            P[:, 2] = 0
        ids = (rng.permutation(n).astype(np.int64) * 7 + 1_000_003).astype(np.int32)
        nan_rows = np.sort(rng.choice(n, min(3, n // 15), replace=False)) if n >= 15 else np.zeros(0, np.int64)
        for t, r in enumerate(nan_rows):
            P[r, (t + n) % 3] = np.nan
        for a in (P, ids, nan_rows):
            a.setflags(write=False)
        _points[key] = (P, ids, nan_rows)
    return _points[key]


def _finite_rows(P):
    return np.flatnonzero(~np.isnan(P).any(axis=1))


def _around(rng, centres, width):
    """One closed box around each centre: it reaches up to `width` to either side, on every axis by another random share."""
    centres = np.asarray(centres, np.float32).reshape(-1, 3)
    lo = centres - (rng.random(centres.shape) * width).astype(np.float32)
    hi = centres + (rng.random(centres.shape) * width).astype(np.float32)
    return np.concatenate([lo, hi], axis=1).astype(np.float32)


def _width(n):
    # boxes hold their centre point at every n; at the large sizes the selected rows stay a minority
    return 0.3 if n < 1000 else 0.06


def _boxes(family, n, P, rng):
    """(boxes (m,6) float32, box_peer (m,) int32, npeers, extra) of a family on the points P."""
    live = _finite_rows(P)
    extra = {}
    if family == "scattered":  # 40 small boxes over 5 peers, peer 2 without one
        boxes = _around(rng, P[rng.choice(live, 40)], _width(n))
        peer = rng.integers(0, 5, 40)
        peer[peer == 2] = 3
        return boxes, peer, 5, extra
    if family == "peers_apart":  # the ends and the middle of the 64-bit peer mask: bits 0, 1, 31, 32, 33, 62, 63
        peer = np.repeat(PEERS_APART, 2)
        return _around(rng, P[rng.choice(live, len(peer))], _width(n)), peer, 64, extra
    if family == "peers_all":  # 64 peers, one box each, every box around the same point
        c = int(rng.choice(live))
        boxes = _around(rng, np.repeat(P[c][None, :], 64, axis=0), _width(n))
        extra["centre"] = c
        return boxes, rng.permutation(64), 64, extra
    if family in ("everything_max", "everything_inf"):
        top = FLT_MAX if family == "everything_max" else np.float32(np.inf)
        boxes = np.tile(np.float32([-top, -top, -top, top, top, top]), (3, 1))
        return boxes, np.arange(3), 3, extra
    if family == "overlaps":
        # peer 1: five nested and shifted boxes over one cluster of points; peers 0, 2, 3, 5: the same region each; peer 4: none
        c = P[int(rng.choice(live))]
        w = np.float32(_width(n))
        nested = [np.concatenate([c - w * f, c + w * f]) for f in (1.0, 0.7, 0.4)]
        shifted = [np.concatenate([c - w * np.float32([1.5, 0.2, 0.2]), c + w * np.float32([0.2, 1.5, 0.2])]),
                   np.concatenate([c - w * np.float32([0.1, 0.1, 1.2]), c + w * np.float32([1.2, 0.1, 0.1])])]
        region = np.concatenate([c - w * np.float32(0.9), c + w * np.float32(0.8)])
        boxes = np.float32(nested + shifted + [region] * 4)
        return boxes, np.int64([1] * 5 + [0, 2, 3, 5]), 6, extra
    if family == "degenerate":
        c = int(rng.choice(live))
        on_point = np.concatenate([P[c], P[c]])  # peer 0: hi == lo on a point's own coordinates: the bounds are closed
        off = np.float32([0.123, 0.456, 0.789])
        assert not (P == off).all(axis=1).any()
        off_point = np.concatenate([off, off])  # peer 1: hi == lo where no point is
        big = np.float32(2)
        inverted = np.float32([-big, 0.75, -big, big, 0.25, big])  # peer 2: lo > hi on the y axis, everything on the others
        nan_bound = np.float32([-big, -big, -big, big, np.nan, big])  # peer 3
        nan_low = np.float32([np.nan, -big, -big, big, big, big])  # peer 3 again
        plain = _around(rng, P[c], _width(n))[0]  # peer 4: an ordinary box, so that something else is selected too
        extra["centre"] = c
        return np.float32([on_point, off_point, inverted, nan_bound, nan_low, plain]), np.int64([0, 1, 2, 3, 3, 4]), 5, extra
    if family == "no_boxes":
        return np.zeros((0, 6), np.float32), np.zeros(0, np.int64), 3, extra
    if family == "one_peer":
        return _around(rng, P[rng.choice(live, 6)], _width(n)), np.zeros(6, np.int64), 1, extra
    if family == "planar":  # z = 0 throughout, boxes whose z range is [0, 0]
        boxes = _around(rng, P[rng.choice(live, 12)], _width(n))
        boxes[:, 2] = 0
        boxes[:, 5] = 0
        return boxes, rng.integers(0, 3, 12), 3, extra
    raise KeyError(family)


_cases = {}


def selection_case(family, n):
    """dict(name, P, ids, nan_rows, boxes, box_peer, npeers, lists, counts, boundary[, centre]) of a family at n points: lists,
    counts and boundary are select's, computed once and shared (do not write to them)."""
    key = (family, n)
    if key not in _cases:
        P, ids, nan_rows = points(n, planar=family == "planar")
        rng = np.random.default_rng(7100 + 31 * FAMILIES.index(family) + n)
        boxes, peer, npeers, extra = _boxes(family, n, P, rng)
        boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
        peer = np.ascontiguousarray(peer, np.int32)
        lists, boundary = select(P, ids, boxes, peer, npeers)
        c = dict(name="%s_n%d" % (family, n), family=family, n=n, P=P, ids=ids, nan_rows=nan_rows, boxes=boxes, box_peer=peer,
                 npeers=npeers, lists=lists, counts=np.int64([len(l) for l in lists]), boundary=boundary, **extra)
        for a in [boxes, peer, boundary, c["counts"]] + lists:
            a.setflags(write=False)
        _cases[key] = c
    return _cases[key]


def capacities(counts, shift):
    """Per-peer capacities of a fixed-capacity case, from the spec's own counts: peer p is given, by (p + shift) % 5,
    0 | count - 1 | count | count + 1 | an ample 2 * count + 3 rows."""
    counts = np.asarray(counts, np.int64)
    mode = (np.arange(len(counts)) + shift) % 5
    caps = np.select([mode == 0, mode == 1, mode == 2, mode == 3], [0 * counts, np.maximum(counts - 1, 0), counts, counts + 1],
                     2 * counts + 3)
    return caps.astype(np.int64)


def fixed_cases():
    """[(selection case, caps)] of the one-pass form: the families FIXED_FAMILIES at the sizes FIXED_N.  The shift of the capacity
    pattern moves with the case, so that every peer position meets every kind of capacity."""
    out = []
    for f, family in enumerate(FIXED_FAMILIES):
        for s, n in enumerate(FIXED_N):
            c = selection_case(family, n)
            out.append((c, capacities(c["counts"], 1 + f + s)))
    return out


def row_of_id(ids):
    """A function id array -> row array for the distinct ids `ids`."""
    ids = np.asarray(ids)
    order = np.argsort(ids, kind="stable")
    sorted_ids = ids[order]

    def rows(some):
        some = np.asarray(some)
        at = np.searchsorted(sorted_ids, some)
        at = np.minimum(at, len(sorted_ids) - 1) if len(sorted_ids) else at
        assert len(some) == 0 or np.array_equal(sorted_ids[at], some), "an id that no row carries"
        return order[at]
    return rows


# ---- segment minimum ------------------------------------------------------------------------------------------------------------

def segment_min(segment, value, out):
    """A copy of `out` with out[s] = min(out[s], value[i]) over the entries with segment[i] == s >= 0."""
    segment, value = np.asarray(segment, np.int64), np.asarray(value, np.int64)
    res = np.array(out, np.int64, copy=True)
    live = segment >= 0
    np.minimum.at(res, segment[live], value[live])
    return res


SEGMENT_N = (0, 1, 63, 64, 65, 255, 256, 257, 100_003)
LAYOUTS = ("one", "two", "three", "five", "sixty_four", "runs", "none", "mixed")
MULTI_LAYOUTS = ("three", "five", "sixty_four")
VALUES = ("small", "negative", "above_2_32", "above_2_53", "extremes", "equal")
PRESETS = ("max", "minimum", "below", "random")


def layout(name, n, rng):
    """(segment (n,) int32, m): m the length of `out`; some segments below m are named by no entry."""
    i = np.arange(n)
    if name == "one":
        return np.zeros(n, np.int32), 1
    if name == "two":  # interleaved lane by lane; segment 2 is named by nobody
        return (i % 2).astype(np.int32), 3
    if name == "three":
        return (i % 3).astype(np.int32), 3
    if name == "five":  # the segments 0, 14, 28, 42, 56 of 70
        return (i % 5 * 14).astype(np.int32), 70
    if name == "sixty_four":
        return (i % 64 + 3).astype(np.int32), 70
    if name == "runs":  # runs of equal segments, 1 to 200 long, numbered at random below 5 000
        lengths = rng.integers(1, 201, n + 1)
        seg = np.repeat(rng.integers(0, 5000, len(lengths)), lengths)[:n]
        return seg.astype(np.int32), 5000
    if name == "none":
        return np.full(n, -1, np.int32), 3
    if name == "mixed":  # a random 30 % of the entries are -1
        seg = rng.integers(0, 70, n)
        seg[rng.random(n) < 0.3] = -1
        return seg.astype(np.int32), 70
    raise KeyError(name)


def values(name, n, rng):
    """(n,) int64"""
    if name == "small":
        return rng.integers(0, 1000, n).astype(np.int64)
    if name == "negative":
        return -rng.integers(1, 10 ** 12, n).astype(np.int64)
    if name == "above_2_32":  # equal above bit 3: a comparison of the high words alone cannot order them
        return (1 << 40) + rng.integers(0, 8, n).astype(np.int64)
    if name == "above_2_53":  # no double tells them apart
        return (1 << 60) + rng.integers(0, 8, n).astype(np.int64)
    if name == "extremes":
        return rng.choice(np.int64([I64_MIN, I64_MAX, I64_MAX - 1, I64_MIN + 1, 0, -1, 1]), n).astype(np.int64)
    if name == "equal":
        return np.full(n, 7, np.int64)
    raise KeyError(name)


def preset(name, segment, value, m, rng):
    """(m,) int64: what `out` holds before the call."""
    if name == "max":
        return np.full(m, I64_MAX, np.int64)
    if name == "minimum":  # already the result
        return segment_min(segment, value, np.full(m, I64_MAX, np.int64))
    if name == "below":  # nothing is smaller: the call must leave it
        return np.full(m, I64_MIN, np.int64)
    if name == "random":  # per entry a value of the family itself or the result, so that some entries fall and some stay
        pool = value if len(value) else np.int64([0])
        truth = segment_min(segment, value, np.full(m, I64_MAX, np.int64))
        return np.where(rng.random(m) < 0.5, truth, rng.choice(pool, m)).astype(np.int64)
    raise KeyError(name)


def segment_combos():
    """The (n, layout, values, preset) the GPU test runs, listed: every size with every layout (72), the value family and the
    preset moving with both so that every (layout, values), (layout, preset) and (values, preset) pair occurs at a size of 63 or
    more.  At every size each preset goes to one of the layouts (three, five, sixty_four, mixed), whose waves hold three and more
    segments, and to one of the other four."""
    rank = {"one": 0, "two": 1, "runs": 2, "none": 3, "three": 0, "five": 1, "sixty_four": 2, "mixed": 3}
    return [(n, lay, VALUES[(5 * li + ni) % len(VALUES)], PRESETS[(rank[lay] + ni) % len(PRESETS)])
            for ni, n in enumerate(SEGMENT_N) for li, lay in enumerate(LAYOUTS)]


def segment_case(n, lay, val, pre):
    """dict(segment, value, out, m, want) of a combination; want = segment_min(segment, value, out)."""
    rng = np.random.default_rng([8000, n, LAYOUTS.index(lay), VALUES.index(val), PRESETS.index(pre)])
    segment, m = layout(lay, n, rng)
    value = values(val, n, rng)
    out = preset(pre, segment, value, m, rng)
    return {"segment": segment, "value": value, "out": out, "m": m, "want": segment_min(segment, value, out)}


# ---- tknnDbscanAssign -----------------------------------------------------------------------------------------------------------

ASSIGN_SETS = ("mixture", "slabs", "nan", "edges", "n1", "n2", "n255", "n256", "n257")
TOP_LABEL = 2 ** 31 - 1
_assign = {}


def remapped(labels, core, clusters):
    """core_label (n,) int32: cluster c of the oracle becomes TOP_LABEL - c * step -- order-reversing, with gaps, cluster 0 at
    2**31 - 1 --, a point that is not core -1."""
    step = min(1_000_003, TOP_LABEL // max(int(clusters), 1))
    remap = TOP_LABEL - np.arange(max(int(clusters), 1), dtype=np.int64) * step
    return np.where(core, remap[np.maximum(labels, 0)], -1).astype(np.int32)


def assign_case(name):
    """dict(name, P, ids, eps, core, core_label, want) of a named set: the sets of dbscan_query_spec (the points of `edges` are
    those of its first case) and small mixtures of 1, 2, 255, 256 and 257 points.  core: oracle.dbscan's flags; core_label:
    remapped(); want (n,) int32: core rows keep their label, every other row is query_labels' -- brute force over all pairs,
    computed once and shared."""
    if name not in _assign:
        if name in dq.SET_NAMES:
            c = dq.cases(name)[0]
            P, eps, ref = c["P"], c["eps"], c["oracle"]
        else:
            n = int(name[1:])
            P = np.ascontiguousarray(datasets.gaussian_mixture3d(n, components=2, sigma=0.02, seed=50 + n), np.float32)
            eps = float(np.float32(0.02))
            ref = oracle.dbscan(P, eps, 3 if n > 2 else 1)
        core = ref["core"].astype(bool)
        core_label = remapped(ref["labels"], core, ref["clusters"])
        want = core_label.copy()
        rest = np.flatnonzero(~core)
        want[rest] = dq.query_labels(P, core_label, eps, P[rest])[0]
        ids = (np.random.default_rng(9000 + len(P)).permutation(len(P)).astype(np.int64) * 5 + 2_000_003).astype(np.int32)
        for a in (core, core_label, want, ids):
            a.setflags(write=False)
        _assign[name] = dict(name=name, P=P, ids=ids, eps=eps, core=core, core_label=core_label, want=want, oracle=ref)
    return _assign[name]
