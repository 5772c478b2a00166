"""tests/lbvh_spec.py (the numpy statement of what the LBVH builder must produce, which tests/test_lbvh_gpu.py compares
the device's arrays with) held against brute force: explicit member lists, explicit walks, bit-by-bit prefixes of Python
integers.  No GPU.  One mutation check per property: a nudged value must be reported by lbvh_spec.compare, the function
the GPU test asserts with."""
import numpy as np
import pytest

import lbvh_spec as ls

END = int(ls.END)
SIZES = [1, 2, 3, 17, 100, 1100]
CURVES = [ls.HILBERT, ls.MORTON]


def _points(n, seed=0):
    """Clustered points with a run of duplicates and one NaN point (where n allows)."""
    rng = np.random.default_rng(seed + n)
    centres = rng.random((4, 3), dtype=np.float32)
    p = (centres[rng.integers(0, 4, n)] + rng.normal(0, 0.03, (n, 3)).astype(np.float32)).astype(np.float32)
    if n >= 17:
        p[5:5 + n // 8] = p[2]
    if n >= 3:
        p[n // 2, 1] = np.nan
    return p


_cache = {}


def _spec(n, curve):
    if (n, curve) not in _cache:
        p = _points(n)
        s = ls.build_points(p, curve=curve)
        for a in s.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[(n, curve)] = (p, s)
    return _cache[(n, curve)]


def _decode(s):
    nodes = s["nodes"]
    split, other = nodes[:, 3].view(np.int32).astype(np.int64), nodes[:, 7].view(np.int32).astype(np.int64)
    i = np.arange(len(nodes))
    return split, np.minimum(i, other), np.maximum(i, other), nodes[:, 0:3].view(np.float32), nodes[:, 4:7].view(np.float32)


def _children(v, split, first, last):
    left = ~split[v] if first[v] == split[v] else split[v]
    right = ~(split[v] + 1) if last[v] == split[v] + 1 else split[v] + 1
    return int(left), int(right)


def _members(s):
    """Per internal node the sorted slots of the leaves below it, by walking child references from the root."""
    split, first, last, _, _ = _decode(s)
    members = {}

    def below(ref):
        if ref < 0:
            return [~ref]
        left, right = _children(ref, split, first, last)
        members[ref] = below(left) + below(right)
        return members[ref]

    if s["n"] > 1:
        below(0)
    return members


def _stored(s):
    pts = s["points"][: s["n"], :3].view(np.float32)
    return pts


def _brute_box(pts):
    lo, hi = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
    for p in pts:
        for a in range(3):
            if p[a] == p[a]:
                lo[a], hi[a] = min(lo[a], p[a]), max(hi[a], p[a])
    return lo, hi


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", SIZES)
def test_leaves_under_a_node_are_its_range_and_its_box_is_theirs(n, curve):
    _, s = _spec(n, curve)
    split, first, last, lo, hi = _decode(s)
    members = _members(s)
    assert sorted(members) == list(range(n - 1)), "not every node id is reached from the root exactly once"
    pts = _stored(s)
    for v, m in members.items():
        assert m == list(range(first[v], last[v] + 1)), v
        blo, bhi = _brute_box(pts[m])
        assert np.array_equal(lo[v].view(np.uint32), blo.view(np.uint32)) and np.array_equal(hi[v].view(np.uint32), bhi.view(np.uint32)), v
    if n > 1:
        assert first[0] == 0 and last[0] == n - 1
        assert np.array_equal(s["split_owner"][split], np.arange(n - 1))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", SIZES)
def test_order_keys_and_point_records(n, curve):
    p, s = _spec(n, curve)
    keys, prim = s["keys"], s["prim_id"]
    assert sorted(prim.tolist()) == list(range(n))
    for i in range(n - 1):  # ascending, equal keys in input order
        assert keys[i] < keys[i + 1] or (keys[i] == keys[i + 1] and prim[i] < prim[i + 1])
    assert np.array_equal(s["row_slot"][prim], np.arange(n))
    bad = np.isnan(p).any(axis=1)
    assert s["nan_count"] == bad.sum() and np.all(bad[prim[n - s["nan_count"]:]]) and not np.any(bad[prim[: n - s["nan_count"]]])
    rec = s["points"]
    assert len(rec) == (n + 15) // 16 * 16 + 16
    assert np.array_equal(rec[:n, 3].view(np.int32), prim)
    want = np.ascontiguousarray(p[prim]).view(np.uint32).copy()
    want[bad[prim]] = 0x7fc00000
    assert np.array_equal(rec[:n, :3], want)
    assert np.all(rec[n:, :3] == 0x7fc00000) and np.all(rec[n:, 3].view(np.int32) == -1)
    good = p[~bad]
    assert np.array_equal(s["scene"], np.concatenate([good.min(0), good.max(0)]))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", SIZES)
def test_the_tree_is_the_radix_tree_of_key_and_position(n, curve):
    """Karras' conditions on Python integers: with a(i) = key(i) * 2^32 + i, a node's range shares a strictly longer prefix
    than it does with either outer neighbour, and its split is the last position that shares more than the range's prefix
    with the first."""
    _, s = _spec(n, curve)
    split, first, last, _, _ = _decode(s)
    a = [(int(k) << 32) | i for i, k in enumerate(s["keys"])]

    def prefix(i, j):
        return 96 - (a[i] ^ a[j]).bit_length()

    for v in range(n - 1):
        f, l, sp = int(first[v]), int(last[v]), int(split[v])
        d = prefix(f, l)
        assert f == 0 or prefix(f - 1, l) < d
        assert l == n - 1 or prefix(f, l + 1) < d
        assert prefix(f, sp) > d or sp == f
        assert prefix(f, sp + 1) == d
    # node numbering: a left child is its range's last position, a right child its first
    for v in range(n - 1):
        left, right = _children(v, split, first, last)
        if left >= 0:
            assert left == last[left] and first[left] == first[v]
        if right >= 0:
            assert right == first[right] and last[right] == last[v]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", SIZES)
def test_rope_walks(n, curve):
    _, s = _spec(n, curve)
    split, first, last, _, _ = _decode(s)
    rope_node, rope_leaf = s["rope_node"], s["rope_leaf"]
    # always descend: the leaves 0 .. n-1 in order
    ref, seen = (0 if n > 1 else ~0), []
    while ref != END:
        assert len(seen) <= n
        if ref >= 0:
            ref = _children(ref, split, first, last)[0]
        else:
            seen.append(~ref)
            ref = int(rope_leaf[~ref])
    assert seen == list(range(n))

    # never descend from v: the walk resumes at the first leaf after v's range
    def first_leaf(ref):
        while ref >= 0:
            ref = _children(ref, split, first, last)[0]
        return ~ref

    for v in range(n - 1):
        r = int(rope_node[v])
        assert (r == END and last[v] == n - 1) or (r != END and first_leaf(r) == last[v] + 1), v
        if r >= 0:
            assert first[r] == last[v] + 1
    for p in range(n):
        r = int(rope_leaf[p])
        assert (r == END and p == n - 1) or (r != END and first_leaf(r) == p + 1), p


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", SIZES + [1025, 70_000])
def test_wide_pyramid_entries_are_the_union_of_their_children(n, curve):
    if n > 1100:
        s = ls.build_points(_points(n), curve=curve)
    else:
        _, s = _spec(n, curve)
    count, boxes = s["wide_count"], s["wide_boxes"]
    levels = s["wide_levels"]
    assert count[0] == (n + 15) // 16 and np.all(count[levels:] == 0) and count[levels - 1] <= 64
    assert all(count[l] == (count[l - 1] + 63) // 64 and count[l - 1] > 64 for l in range(1, levels))
    assert len(boxes) == count.sum()
    pts = _stored(s)
    at = 0
    for b in range(count[0]):
        lo, hi = _brute_box(pts[16 * b: 16 * b + 16])
        assert np.array_equal(boxes[b].view(np.uint32), np.concatenate([lo, hi]).view(np.uint32)), b
    for l in range(1, levels):
        below, at = boxes[at: at + count[l - 1]], at + count[l - 1]
        for j in range(count[l]):
            kids = below[64 * j: 64 * j + 64]
            want = np.concatenate([kids[:, :3].min(0), kids[:, 3:].max(0)])
            assert np.array_equal(boxes[at + j].view(np.uint32), want.view(np.uint32)), (l, j)


def test_box_trees_key_on_centres_and_bound_their_boxes():
    rng = np.random.default_rng(4)
    lo = rng.random((300, 3), dtype=np.float32)
    boxes = np.concatenate([lo, lo + rng.random((300, 3), dtype=np.float32) * np.float32(0.1)], 1)
    moved = boxes + np.float32(0.25)
    for refit in (None, moved):
        s = ls.build_boxes(boxes, refit=refit)
        now = boxes if refit is None else moved
        assert np.array_equal(s["sorted_boxes"], now[s["prim_id"]])
        split, first, last, nlo, nhi = _decode(s)
        for v in range(299):
            m = now[s["prim_id"][first[v]: last[v] + 1]]
            assert np.array_equal(nlo[v], m[:, :3].min(0)) and np.array_equal(nhi[v], m[:, 3:].max(0))
    same = ls.build_boxes(boxes)
    assert not ls.compare(s, same, ("keys", "prim_id", "rope_node", "rope_leaf"))  # a refit keeps order and topology
    assert np.array_equal(s["nodes"][:, [3, 7]], same["nodes"][:, [3, 7]])
    # a box degenerate to a point keys like the point
    p = _points(100)[:40]  # (no NaN in there)
    assert np.array_equal(ls.build_boxes(np.concatenate([p, p], 1))["prim_id"], ls.build_points(p)["prim_id"])


# ---- the comparison the GPU test asserts with reports each kind of fault ----
def _nudged(s, name, index, how):
    t = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    if isinstance(t[name], np.ndarray):
        t[name][index] = how(t[name][index])
    else:
        t[name] = how(t[name])
    return t


MUTATIONS = [
    ("a node box too large", "nodes", (40, 4), lambda w: w + 1),  # hi.x one ulp up
    ("a split in another place", "nodes", (40, 3), lambda w: w ^ 1),
    ("a node's other end", "nodes", (7, 7), lambda w: w + 1),
    ("a leaf's rope", "rope_leaf", 11, lambda w: ~w),
    ("a node's rope", "rope_node", 11, lambda w: w + 1),
    ("a wide entry too large", "wide_boxes", (3, 5), lambda w: np.nextafter(w, np.float32(np.inf))),
    ("a wide level too many", "wide_levels", None, lambda w: w + 1),
    ("a stale wide count", "wide_count", 2, lambda w: w + 1),
    ("a key", "keys", 5, lambda w: w ^ np.uint64(1)),
    ("two slots swapped in the order", "prim_id", slice(20, 22), lambda w: w[::-1]),
    ("row_slot not the inverse", "row_slot", slice(20, 22), lambda w: w[::-1]),
    ("a sentinel that is a point", "points", (1100, 0), lambda w: np.uint32(0)),
    ("a NaN point stored as given", "points", (1099, 0), lambda w: np.uint32(0x3f800000)),
    ("an id", "points", (3, 3), lambda w: w + 1),
    ("the scene box", "scene", 4, lambda w: np.nextafter(w, np.float32(np.inf))),
    ("the NaN count", "nan_count", None, lambda w: w + 1),
    ("a split's owner", "split_owner", 9, lambda w: w + 1),
]


@pytest.mark.parametrize("what, name, index, how", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_compare_reports_a_nudged_value(what, name, index, how):
    _, s = _spec(1100, ls.HILBERT)
    assert ls.compare(s, s) == []
    wrong = ls.compare(_nudged(s, name, index, how), s)
    assert len(wrong) == 1 and wrong[0].startswith(name + "["), wrong


def test_compare_reports_shape_type_and_missing_fields():
    _, s = _spec(100, ls.HILBERT)
    t = dict(s)
    t["rope_leaf"] = s["rope_leaf"][:-1]
    t["keys"] = s["keys"].astype(np.uint32)
    del t["scene"]
    assert sorted(w.split("[")[0] for w in ls.compare(t, s)) == ["keys", "rope_leaf", "scene"]
    # -0.0 is not +0.0 here: floats compare as bit patterns
    t = dict(s)
    t["scene"] = s["scene"].copy()
    t["scene"][0] = np.float32(0.0)
    u = dict(t)
    u["scene"] = t["scene"].copy()
    u["scene"][0] = np.float32(-0.0)
    assert ls.compare(u, t, ("scene",)) == ["scene[0]"]
