"""What the LBVH builder (owlraytracing_amd/csrc/lbvh.hip) must produce, restated in numpy from the header comments of
include/owl/lbvh_device.h, owlraytracing_amd/csrc/lbvh.h and curve_key.h.  No tests here: tests/test_lbvh_expectations.py
holds this file against brute force on the CPU, tests/test_lbvh_gpu.py holds the builder against this file.

  * scene box: fmin / fmax over the input (NaN ignored); ext = the largest extent, in float32.
  * keys: curve_point_key(curve, point, scene lo, ext, 21 levels), taken from the host-compiled curve_key.h
    (tests/curve_key_host.py; tests/test_curve_key.py checks that function itself).  Box trees key on the centre
    0.5f*lo + 0.5f*hi, each operation rounded to float32.
  * order: the stable order of the keys.
  * tree: the radix tree of the keys, equal keys told apart by position.  A range [first, last] splits after the last
    position whose (key, position) agrees with first's in the highest bit in which first's and last's differ.  A range
    that is a left child is node `last`, a right child is node `first`, the root is node 0; node.other is the range's
    other end.
  * node box: fmin / fmax over the sorted range; a point with a NaN coordinate is stored all-NaN and widens nothing; a
    range of such points alone is (+inf, -inf).
  * ropes: of a left child its right sibling, of a right child its parent's rope, of the root LBVH_END; references are
    node ids, or ~slot for leaves.
  * wide pyramid: level 0 = the boxes of the runs of 16 sorted points (the last may be short), level l = the boxes of
    64 entries of level l-1; levels are added while the top has more than 64 entries, up to 6.
  * points: the sorted points {x, y, z, id}, id = ids[row] or the row; then sentinels {NaN, NaN, NaN, -1} up to
    ceil(n/16)*16 + 16 records.  row_slot = the inverse of the order; nan_count = the points with a NaN coordinate.

The tree is built level by level, every range of one depth at once (they are disjoint, so np.minimum.reduceat gives
their boxes): nothing here follows the device's per-node search.
"""
import numpy as np

import curve_key_host
from curve_key_host import HILBERT, MORTON  # noqa: F401

END = np.int32(-2**31)
BLOCK, WIDE_LEVELS, KEY_LEVELS = 16, 6, 21
NAN_BITS = np.uint32(0x7fc00000)


def pad3(points):
    p = np.asarray(points, np.float32)
    if p.shape[1] == 2:
        p = np.concatenate([p, np.zeros((len(p), 1), np.float32)], axis=1)
    return np.ascontiguousarray(p)


def bit_length(v):
    v = np.asarray(v).astype(np.uint64)
    out = np.zeros(v.shape, np.int64)
    for sh in (32, 16, 8, 4, 2, 1):
        big = (v >> np.uint64(sh)) != 0
        out += np.where(big, sh, 0)
        v = np.where(big, v >> np.uint64(sh), v)
    return out + (v != 0)


def scene_box(lo, hi):
    """(6 floats: lo xyz, hi xyz; ext) of primitives with lower corners ``lo`` and upper corners ``hi``."""
    s_lo = np.fmin.reduce(lo, axis=0, initial=np.float32(np.inf)).astype(np.float32)
    s_hi = np.fmax.reduce(hi, axis=0, initial=np.float32(-np.inf)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        d = (s_hi - s_lo).astype(np.float32)
    ext = np.fmax(np.fmax(d[0], d[1]), d[2]).astype(np.float32)
    return np.concatenate([s_lo, s_hi]), ext


def radix_tree(keys):
    """dict(split, other (n-1), rope_node (n-1), rope_leaf (n), split_owner (n-1), levels) of sorted uint64 ``keys``;
    levels: per depth (node ids, first, last) of that depth's internal nodes, ascending."""
    keys = np.asarray(keys, np.uint64)
    n = len(keys)
    m = max(n - 1, 0)
    split, other = np.zeros(m, np.int64), np.zeros(m, np.int64)
    rope_node, rope_leaf = np.full(m, END, np.int64), np.full(n, END, np.int64)
    levels = []
    ids, f, l, rope = (np.zeros(min(m, 1), np.int64), np.zeros(min(m, 1), np.int64), np.full(min(m, 1), n - 1, np.int64),
                       np.full(min(m, 1), END, np.int64))
    while len(ids):
        levels.append((ids, f, l))
        kf, kl = keys[f], keys[l]
        same = kf == kl
        b = np.where(same, bit_length(f ^ l), bit_length(kf ^ kl)) - 1  # the highest bit in which the two ends differ
        bu = b.astype(np.uint64)
        # first's bit b is 0 and last's is 1: the split is before the first (key, position) with that bit set
        by_key = np.searchsorted(keys, ((kf >> bu) + np.uint64(1)) << bu, side="left") - 1
        by_pos = (((f >> b) + 1) << b) - 1
        s = np.where(same, by_pos, by_key)
        assert np.all((s >= f) & (s < l))
        split[ids] = s
        other[ids] = np.where(ids == f, l, f)
        left_inner, right_inner = f < s, s + 1 < l
        right_ref = np.where(right_inner, s + 1, ~(s + 1))
        rope_node[s[left_inner]] = right_ref[left_inner]
        rope_leaf[f[~left_inner]] = right_ref[~left_inner]
        rope_node[(s + 1)[right_inner]] = rope[right_inner]
        rope_leaf[l[~right_inner]] = rope[~right_inner]
        nf, nl = np.stack([f, s + 1], 1).ravel(), np.stack([s, l], 1).ravel()
        nid, nrope = np.stack([s, s + 1], 1).ravel(), np.stack([right_ref, rope], 1).ravel()
        inner = nf < nl
        ids, f, l, rope = nid[inner], nf[inner], nl[inner], nrope[inner]
    split_owner = np.zeros(m, np.int64)
    split_owner[split] = np.arange(m)
    return {"split": split, "other": other, "rope_node": rope_node.astype(np.int32), "rope_leaf": rope_leaf.astype(np.int32),
            "split_owner": split_owner.astype(np.int32), "levels": levels}


def _reduce_runs(lo, hi, starts, ends):
    """Boxes of the disjoint ascending runs [starts[i], ends[i]) of rows of lo / hi."""
    pad = np.full((1, 3), np.inf, np.float32)
    idx = np.stack([starts, ends], 1).ravel()
    return (np.minimum.reduceat(np.concatenate([lo, pad]), idx, axis=0)[0::2],
            np.maximum.reduceat(np.concatenate([hi, -pad]), idx, axis=0)[0::2])


def node_table(tree, lo, hi):
    """(n-1, 8) uint32: {lo[3], split, hi[3], other} per internal node, boxes over the sorted primitive corners lo / hi
    (NaN rows already turned into +inf / -inf)."""
    m = len(tree["split"])
    nodes = np.zeros((m, 8), np.uint32)
    nodes[:, 3] = tree["split"].astype(np.int32).view(np.uint32)
    nodes[:, 7] = tree["other"].astype(np.int32).view(np.uint32)
    for ids, f, l in tree["levels"]:
        blo, bhi = _reduce_runs(lo, hi, f, l + 1)
        nodes[ids, 0:3] = blo.view(np.uint32)
        nodes[ids, 4:7] = bhi.view(np.uint32)
    return nodes


def wide_pyramid(lo, hi):
    """(levels, count[6], boxes (sum of counts, 6) float32) over the sorted points' corners."""
    counts, boxes = [], []
    while True:
        width = BLOCK if not counts else 64
        starts = np.arange(0, len(lo), width)
        lo, hi = _reduce_runs(lo, hi, starts, np.minimum(starts + width, len(lo)))
        counts.append(len(lo))
        boxes.append(np.concatenate([lo, hi], 1))
        if len(lo) <= 64 or len(counts) == WIDE_LEVELS:
            break
    return len(counts), np.array(counts + [0] * (WIDE_LEVELS - len(counts)), np.int32), np.concatenate(boxes)


def _keys_and_order(centres, scene, ext, curve):
    keys = curve_key_host.point_keys(curve_key_host.load(), curve, KEY_LEVELS, centres, scene[:3], ext)
    order = np.argsort(keys, kind="stable")
    return keys[order], order


def build_points(points, ids=None, curve=HILBERT):
    """Everything TrueKNN.export_tree_ex returns for build(points, ids) under that curve."""
    p = pad3(points)
    n = len(p)
    scene, ext = scene_box(p, p)
    keys, order = _keys_and_order(p, scene, ext, curve)
    bad = np.isnan(p).any(axis=1)
    tree = radix_tree(keys)
    sp = p[order]
    lo, hi = sp.copy(), sp.copy()
    lo[bad[order]], hi[bad[order]] = np.inf, -np.inf
    total = (n + BLOCK - 1) // BLOCK * BLOCK + BLOCK
    records = np.empty((total, 4), np.uint32)
    records[:, :3], records[:, 3] = NAN_BITS, np.int32(-1).view(np.uint32)
    records[:n, :3] = sp.view(np.uint32)
    records[:n][bad[order], :3] = NAN_BITS
    records[:n, 3] = (order if ids is None else np.asarray(ids)[order]).astype(np.int32).view(np.uint32)
    row_slot = np.empty(n, np.int32)
    row_slot[order] = np.arange(n, dtype=np.int32)
    levels, count, wide = wide_pyramid(lo, hi)
    return {"n": n, "curve": int(curve), "keys": keys, "prim_id": order.astype(np.int32), "row_slot": row_slot, "points": records,
            "scene": scene, "nan_count": int(bad.sum()), "nodes": node_table(tree, lo, hi), "rope_node": tree["rope_node"],
            "rope_leaf": tree["rope_leaf"], "split_owner": tree["split_owner"], "wide_levels": levels, "wide_count": count,
            "wide_boxes": wide}


def build_boxes(boxes, curve=HILBERT, refit=None):
    """What tknnDebugBoxTree returns for (n, 6) float32 ``boxes`` {lo xyz, hi xyz}: order and topology from ``boxes``, node
    boxes and sorted_boxes from ``refit`` where one is given."""
    b = np.ascontiguousarray(boxes, np.float32)
    scene, ext = scene_box(b[:, :3], b[:, 3:])
    half = np.float32(0.5)
    centres = (half * b[:, :3] + half * b[:, 3:]).astype(np.float32)
    keys, order = _keys_and_order(centres, scene, ext, curve)
    tree = radix_tree(keys)
    now = (b if refit is None else np.ascontiguousarray(refit, np.float32))[order]
    return {"n": len(b), "keys": keys, "prim_id": order.astype(np.int32), "nodes": node_table(tree, now[:, :3], now[:, 3:]),
            "rope_node": tree["rope_node"], "rope_leaf": tree["rope_leaf"], "sorted_boxes": now}


def _words(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return a


def compare(got, want, fields=None):
    """The fields of ``want`` (or ``fields``) in which ``got`` differs, as 'name[first differing flat index]' -- empty if
    the two agree word for word (floats are compared as their bit patterns)."""
    wrong = []
    for name in (fields or want.keys()):
        if name not in got:
            wrong.append(name + "[missing]")
            continue
        g, w = _words(np.asarray(got[name])), _words(np.asarray(want[name]))
        if g.shape != w.shape:
            wrong.append("%s[shape %s, expected %s]" % (name, g.shape, w.shape))
        elif g.dtype.itemsize != w.dtype.itemsize or not np.array_equal(g, w):
            at = np.flatnonzero(g.ravel() != w.ravel())
            wrong.append("%s[%s]" % (name, at[0] if len(at) else "type"))
    return wrong
