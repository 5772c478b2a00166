"""What TrueKNN.voxel_down_sample (tknnVoxelGrid, include/owlknn_voxel.h) must give, restated in numpy, and the cases its tests
share.  No tests here.

Cells are computed in np.float32 with the header's literal expression floor((p - origin) / voxel), voxels are ordered by
np.lexsort over (label, cx, cy, cz), the sums run in np.float64 in ascending row order (`reverse`: in descending row order, what
the tests bound the library's own order with), and the nearest row is computed from a centroid that is passed in."""
import numpy as np

CELLS = 1 << 21  # TKNN_VOXEL_CELL_BITS


def cells_of(P, voxel, origin):
    """(cells (n,3) float32 -- floor((p - origin) / voxel), each operation one fp32 one --, finite (n,) bool)."""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    finite = np.isfinite(P).all(axis=1)
    with np.errstate(all="ignore"):
        c = np.floor((P - np.float32(origin).reshape(1, 3)) / np.float32(voxel))
    assert c.dtype == np.float32
    return c, finite


def grid(P, voxel, origin, batch=None, B=1, values=None, reverse=False):
    """dict(V, cells (V,3) int32, counts, first, labels (V,) int32, offsets (B+1,) int64, map (n,) int32, centroid (V,3) float32,
    means (V,C) float32, bad_rows, bad_labels, out_of_grid, rows_in_grid, max_count, members: the rows of every voxel, ascending)."""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    n = len(P)
    c, finite = cells_of(P, voxel, origin)
    label = np.zeros(n, np.int64) if batch is None else np.asarray(batch, np.int64)
    label_ok = (label >= 0) & (label < B)
    with np.errstate(invalid="ignore"):
        inside = ((c >= 0) & (c < CELLS)).all(axis=1)
    bad_rows = ~finite
    bad_labels = finite & ~label_ok
    outside = finite & label_ok & ~inside
    keep = finite & label_ok & inside
    rows = np.flatnonzero(keep)
    ci = c[rows].astype(np.int64)
    order = np.lexsort((rows, ci[:, 2], ci[:, 1], ci[:, 0], label[rows]))  # the last key is the first to decide
    rows, ci, lab = rows[order], ci[order], label[rows][order]
    tup = np.concatenate([lab[:, None], ci], axis=1)
    head = np.ones(len(rows), bool)
    head[1:] = (tup[1:] != tup[:-1]).any(axis=1)
    number = np.cumsum(head) - 1
    V = int(head.sum())
    starts = np.flatnonzero(head)
    members = np.split(rows, starts[1:]) if V else []
    vmap = np.full(n, -1, np.int32)
    vmap[rows] = number
    C = 0 if values is None else np.asarray(values).shape[1]
    centroid, means = np.zeros((V, 3), np.float32), np.zeros((V, C), np.float32)
    values64 = None if values is None else np.asarray(values, np.float32).astype(np.float64)
    P64 = P.astype(np.float64)

    def mean(columns, m):
        s = np.zeros(columns.shape[1], np.float64)
        with np.errstate(all="ignore"):
            for r in (m[::-1] if reverse else m):
                s = s + columns[r]
            return (s / np.float64(len(m))).astype(np.float32)

    for v, m in enumerate(members):
        centroid[v] = mean(P64, m)
        if C:
            means[v] = mean(values64, m)
    counts = np.int32([len(m) for m in members])
    labels = lab[starts].astype(np.int32)
    return {"V": V, "cells": ci[starts].astype(np.int32).reshape(V, 3), "counts": counts, "first": np.int32([m[0] for m in members]), "labels": labels,
            "offsets": np.searchsorted(labels, np.arange(B + 1), side="left").astype(np.int64), "map": vmap, "centroid": centroid, "means": means,
            "bad_rows": int(bad_rows.sum()), "bad_labels": int(bad_labels.sum()), "out_of_grid": int(outside.sum()), "rows_in_grid": int(keep.sum()),
            "max_count": int(counts.max()) if V else 0, "members": members}


def nearest(P, members, centroid):
    """Per voxel the row with the smallest key (bits of d2, row), d2 = (dx*dx + dy*dy) + dz*dz in fp32 against the fp32 centroid
    that is passed in (the library's own, in its tests)."""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    out = np.zeros(len(members), np.int32)
    for v, m in enumerate(members):
        d = P[m] - np.float32(centroid[v])[None, :]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2.dtype == np.float32
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | m.astype(np.uint64)
        out[v] = m[np.argmin(key)]
    return out


def ulps_apart(a, b):
    """How many fp32 values apart the entries of two float32 arrays are (0 where both are NaN)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)

    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    d = np.abs(ordered(a) - ordered(b))
    return np.where(np.isnan(a) & np.isnan(b), 0, d)


# ---- the cases the GPU tests share: name -> dict(P, voxel, origin[, batch, B, values]) --------------------------------------------------
def uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


def cases():
    rng = np.random.default_rng(11)
    out = {}
    zero = (0.0, 0.0, 0.0)
    out["n0"] = dict(P=np.zeros((0, 3), np.float32), voxel=0.5, origin=zero)
    out["n1"] = dict(P=np.float32([[0.3, 0.4, 0.5]]), voxel=0.25, origin=zero)
    out["twins"] = dict(P=np.float32([[0.3, 0.4, 0.5], [0.3, 0.4, 0.5]]), voxel=0.25, origin=zero)
    U = uniform(1025, 5)
    V3 = rng.random((1025, 3), dtype=np.float32)
    out["u1025_one_per_voxel"] = dict(P=U, voxel=0.05, origin=zero, values=V3)  # 8 000 cells: about 1 row per occupied voxel
    out["u1025_128_per_voxel"] = dict(P=U, voxel=0.5, origin=zero, values=V3)  # 8 cells: about 128 rows each, runs over 64
    out["u1025_one_voxel"] = dict(P=U, voxel=2.0, origin=zero, values=V3)  # one run of 1 025 rows: it crosses a workgroup
    # a lattice whose points lie on cell faces: multiples of the voxel, exactly representable
    g = np.arange(7, dtype=np.float32) * np.float32(0.125)
    L = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    out["lattice_on_faces"] = dict(P=np.concatenate([L, L[::3]]), voxel=0.125, origin=zero)
    out["lattice_voxel_quarter"] = dict(P=L, voxel=0.25, origin=(-0.125, 0.0, 0.125))
    # far from zero: the subtraction decides the cell
    F = (np.float32(1000.0) + (rng.random((900, 3), dtype=np.float32) - np.float32(0.5))).astype(np.float32)
    out["at_1000"] = dict(P=F, voxel=0.01, origin=(999.5, 999.5, 999.5))
    # rows that are left out
    M = uniform(600, 6)
    M[5, 0], M[17, 2], M[40, 1], M[41] = np.nan, np.inf, -np.inf, np.nan
    M[100], M[101], M[102] = (-0.001, 0.5, 0.5), (0.5, 3e6, 0.5), (0.5, 0.5, -1e30)
    M[103] = (3e38, 0.5, 0.5)
    mb = rng.integers(0, 3, size=600).astype(np.int32)
    mb[7], mb[8], mb[9], mb[5] = -1, 3, 2 ** 31 - 1, -5  # (row 5 is a bad row first)
    out["left_out"] = dict(P=M, voxel=1.0 / 1024, origin=zero, batch=mb, B=3, values=rng.random((600, 3), dtype=np.float32))
    # three clouds with the same coordinates, the labels shuffled
    T = uniform(300, 7)
    tb = np.repeat(np.arange(3, dtype=np.int32), 300)
    perm = rng.permutation(900)
    out["three_clouds"] = dict(P=np.concatenate([T, T, T])[perm], voxel=0.2, origin=zero, batch=tb[perm], B=3)
    out["empty_clouds"] = dict(P=T, voxel=0.3, origin=zero, batch=np.where(np.arange(300) % 2 == 0, 1, 4).astype(np.int32), B=7)
    # the channels
    W = uniform(700, 8)
    out["c0"] = dict(P=W, voxel=0.25, origin=zero)
    out["c3"] = dict(P=W, voxel=0.25, origin=zero, values=rng.standard_normal((700, 3)).astype(np.float32))
    out["c16"] = dict(P=W, voxel=0.25, origin=zero, values=(rng.standard_normal((700, 16)) * 100).astype(np.float32))
    out["c16_one_voxel"] = dict(P=W, voxel=1.0, origin=zero, values=out["c16"]["values"])
    vals = rng.random((700, 5), dtype=np.float32)
    vals[3, 1], vals[9, 4] = np.nan, np.inf
    out["c5_not_finite"] = dict(P=W, voxel=0.25, origin=zero, values=vals)
    return out


def spec_of(case, reverse=False):
    return grid(case["P"], case["voxel"], case["origin"], case.get("batch"), case.get("B", 1), case.get("values"), reverse=reverse)
