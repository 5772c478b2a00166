"""Point sets full of exact fp32 distance ties, and the tile layouts of the engine's sharded entry surface (tknnBuildIds,
tknnSetHalo, tknnHaloSelect, the phases of tknnSolveEx).  Plain numpy, shared by the GPU tests and by the CPU tests of the
values those expect.

Layouts of a global set G (ids = positions in G, so the replay's tie order by index is the order by id):
  * relabel: local row i holds G[perm[i]] with id perm[i] -- every id below n, none equal to its row;
  * split:   the points on one side of a plane (the tile, in shuffled order) and the rest (the halo, shuffled too);
  * phases:  a split plus the boxes of the sharded driver's first exchange at halo radius r0 * 2**cap.
"""
import numpy as np

from owlraytracing_amd import datasets


def lattice(m, dims, seed, drop=0.2):
    """An m^dims lattice of spacing 1/32 with a share `drop` of its points removed, shuffled."""
    g = np.arange(m, dtype=np.float32) / np.float32(32)
    if dims == 3:
        xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    else:
        xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
        xyz = np.concatenate([xy, np.zeros((len(xy), 1), np.float32)], 1)
    rng = np.random.default_rng(seed)
    xyz = xyz[rng.random(len(xyz)) > drop]
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))])


def quantised_uniform(n, seed):
    """Uniform points rounded to multiples of 1/64."""
    return (np.round(datasets.uniform3d(n, seed=seed) * 64) / 64).astype(np.float32)


def with_duplicates(n, seed, share=0.25):
    """Uniform points of which `share` are copies of others (ties at distance 0 and wherever two copies are listed)."""
    rng = np.random.default_rng(1000 + seed)
    xyz = datasets.uniform3d(n, seed=seed)
    m = int(n * share)
    xyz[rng.choice(n, m, replace=False)] = xyz[rng.integers(0, n, m)]
    return xyz


def tie_set(name):
    """(G, r0) of a named tie set: n <= 4 000."""
    if name == "cross":  # cross-level ties by construction (k = 2, r0 = 1)
        return datasets.cross_round_ties(100), 1.0
    if name == "lattice":
        return lattice(14, 3, 7), 0.02
    if name == "quantised":
        return quantised_uniform(4000, 3), 0.02
    if name == "duplicates":
        return with_duplicates(4000, 4), 0.03
    raise KeyError(name)


def clustered(n=8000):
    """(G, r0): three tight Gaussian clusters, every seventh point a copy of its neighbour, and a start radius far too large
    for the density of the cluster cores -- the packet kernel's lists overflow and its queries are handed over to a tail;
    the sparse fringe needs several levels."""
    xyz = datasets.gaussian_mixture3d(n, components=3, sigma=0.004, seed=13)
    xyz[::7] = xyz[1::7][: len(xyz[::7])]  # duplicates
    return xyz, 0.002


def relabel(n, seed=0):
    """perm: local row i of the relabelled layout holds G[perm[i]] with id perm[i]."""
    return np.random.default_rng(500 + seed).permutation(n).astype(np.int32)


def split(xyz, seed=0, axis=0):
    """(own, rest): positions in G of the points with coordinate `axis` <= the median (the tile) and of the others,
    each in shuffled order (ids not monotone in the local rows)."""
    rng = np.random.default_rng(600 + seed)
    cut = np.float32(np.median(xyz[:, axis]))
    own = np.nonzero(xyz[:, axis] <= cut)[0]
    rest = np.nonzero(xyz[:, axis] > cut)[0]
    return rng.permutation(own).astype(np.int32), rng.permutation(rest).astype(np.int32)


def phase_cap(levels):
    """Halo level of the phase layout: the median of the queries' levels on G, below the largest, so that some queries
    finish within it and some do not."""
    return max(0, min(int(np.median(levels)), int(levels.max()) - 1))


def halo_radius(r0, cap):
    """r0 doubled `cap` times in float32: the radius of level `cap`."""
    r = np.float32(r0)
    for _ in range(cap):
        r = np.float32(r * np.float32(2))
    return r


def widened_box(pts, radius):
    """(6,) float32 closed box lo xyz, hi xyz containing the bounding box of `pts` widened by `radius`, a relative 1e-5
    and 1e-6 of the largest coordinate, rounded OUTWARD -- what the sharded driver hands to tknnHaloSelect."""
    pts = np.asarray(pts, np.float64)
    lo64, hi64 = pts.min(0), pts.max(0)
    mag = max(float(np.abs(lo64).max()), float(np.abs(hi64).max()))
    reach = float(radius) * (1.0 + 1e-5) + 1e-30 + 1e-6 * mag
    lo64, hi64 = lo64 - reach, hi64 + reach
    lo, hi = lo64.astype(np.float32), hi64.astype(np.float32)
    lo = np.where(lo.astype(np.float64) > lo64, np.nextafter(lo, np.float32(-np.inf)), lo)
    hi = np.where(hi.astype(np.float64) < hi64, np.nextafter(hi, np.float32(np.inf)), hi)
    return np.concatenate([lo, hi]).astype(np.float32)


def inside(pts, box):
    """Which points lie in the closed float32 box."""
    pts = np.asarray(pts, np.float32)
    return np.all((box[:3] <= pts) & (pts <= box[3:]), axis=1)


def phases(xyz, own, rest, r0, cap):
    """The first exchange of a tile at halo radius r0 * 2**cap: dict(peer_box: the complement's bounding box widened by
    that radius (the box tknnHaloSelect is given), boundary: per local row, inside it (a boundary query), near: the
    positions in G of the complement's points inside the tile's box widened the same way (the halo of phase 2))."""
    radius = halo_radius(r0, cap)
    peer_box = widened_box(xyz[rest], radius)
    tile_box = widened_box(xyz[own], radius)
    return {"radius": radius, "peer_box": peer_box, "boundary": inside(xyz[own], peer_box),
            "near": rest[inside(xyz[rest], tile_box)]}


def tie_order_needs_level(idx, dist):
    """Per row: does the (distance, id) order of the row differ from its order in the replay ((distance, first level,
    id)) -- a row the tie pass must take the level key for."""
    plain = np.lexsort((idx, dist), axis=1)
    return (plain != np.arange(idx.shape[1])[None, :]).any(axis=1)


def repair_boundary_case():
    """(xyz, r0, k) of a row that is not exact kNN although d_k <= r_q and its own distances are all distinct: query 0 at
    the origin sees (3, 4, 0) at level 0 (box 4.5), and (5, 0, 0) and (0, 0, 4.9) only at level 1 (box 9).  The replay
    keeps [3, 2] (2 was a candidate first); (dist, index) order keeps [3, 1].  Three far-away points finish on their own."""
    xyz = np.float32([[0, 0, 0], [5, 0, 0], [3, 4, 0], [0, 0, 4.9], [50, 50, 50], [51, 50, 50], [50, 52, 50]])
    return xyz, 4.5, 2
