"""The LBVH's sort key (owlraytracing_amd/csrc/curve_key.h), compiled for the host and checked against a numpy restatement
of the Hilbert index written here, and against the properties the tree and the packet kernel rely on:

  * the key is a bijection of the cells, and consecutive keys are face-adjacent cells (what makes it a Hilbert curve);
  * the top 3 m bits of a key are the m-level key of the cell's level-m parent (what the Karras radix tree needs: a
    common key prefix is a common octree cell);
  * a point with a NaN coordinate gets bit 63;
  * sorted along it, blocks of 16 consecutive points have tighter boxes than along the Z curve: a query's box meets
    clearly fewer of them (the block-list model the packet kernel's lists were sized on)."""
import numpy as np
import pytest

import curve_key_host
from curve_key_host import HILBERT, MORTON, keys as _keys, point_keys as _point_keys


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return curve_key_host.compile_shim(tmp_path_factory.mktemp("curve_key"))


# ---- the restatement: bit loops instead of magic masks, whole arrays instead of one cell ----
def np_interleave(x, y, z, levels):
    out = np.zeros(len(x), np.uint64)
    for b in range(levels):
        for shift, v in ((2, x), (1, y), (0, z)):
            out |= ((v.astype(np.uint64) >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + shift)
    return out


def np_hilbert(x, y, z, levels):
    """Skilling's axes-to-transpose, then the transpose read as one number (x's bit first at every level)."""
    X = [np.array(v, dtype=np.uint32) for v in (x, y, z)]
    q = 1 << (levels - 1)
    while q > 1:
        low = np.uint32(q - 1)
        for a in range(3):
            bit = (X[a] & np.uint32(q)) != 0
            swap = np.where(bit, np.uint32(0), (X[0] ^ X[a]) & low)
            X[0] = np.where(bit, X[0] ^ low, X[0]) ^ swap
            if a:
                X[a] = X[a] ^ swap
        q >>= 1
    X[1] = X[1] ^ X[0]
    X[2] = X[2] ^ X[1]
    t = np.zeros(len(X[0]), np.uint32)
    q = 1 << (levels - 1)
    while q > 1:
        t ^= np.where((X[2] & np.uint32(q)) != 0, np.uint32(q - 1), np.uint32(0))
        q >>= 1
    return np_interleave(X[0] ^ t, X[1] ^ t, X[2] ^ t, levels)


def _grid(levels):
    side = 1 << levels
    g = np.arange(side, dtype=np.uint32)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    return x.ravel(), y.ravel(), z.ravel()


def _random_cells(count, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 1 << 21, count, dtype=np.uint32) for _ in range(3))


@pytest.mark.parametrize("levels", [3, 4])
@pytest.mark.parametrize("curve", [HILBERT, MORTON])
def test_whole_grid_bijection_and_restatement(lib, curve, levels):
    x, y, z = _grid(levels)
    key = _keys(lib, curve, levels, x, y, z)
    assert np.array_equal(np.sort(key), np.arange(len(x), dtype=np.uint64)), "not a bijection of the grid's cells"
    want = (np_hilbert if curve == HILBERT else np_interleave)(x, y, z, levels)
    assert np.array_equal(key, want)


@pytest.mark.parametrize("levels", [3, 4])
def test_consecutive_hilbert_keys_are_face_adjacent(lib, levels):
    x, y, z = _grid(levels)
    order = np.argsort(_keys(lib, HILBERT, levels, x, y, z))
    cells = np.stack([x, y, z], 1).astype(np.int64)[order]
    assert np.all(np.abs(np.diff(cells, axis=0)).sum(1) == 1)
    # the Z curve is no such curve: the check above is not vacuous
    order = np.argsort(_keys(lib, MORTON, levels, x, y, z))
    cells = np.stack([x, y, z], 1).astype(np.int64)[order]
    assert np.any(np.abs(np.diff(cells, axis=0)).sum(1) > 1)


def test_random_21_bit_cells(lib):
    x, y, z = _random_cells(200_000, seed=5)
    for curve, restated in ((HILBERT, np_hilbert), (MORTON, np_interleave)):
        key = _keys(lib, curve, 21, x, y, z)
        assert np.array_equal(key, restated(x, y, z, 21))
        assert np.all(key < np.uint64(1) << np.uint64(63))
        # distinct cells, distinct keys
        cells = (x.astype(np.uint64) << np.uint64(42)) | (y.astype(np.uint64) << np.uint64(21)) | z.astype(np.uint64)
        assert len(np.unique(key)) == len(np.unique(cells))
    # neighbours along the 21-level curve: the cell after a random cell's key is face-adjacent.  Walk a short run of the curve
    # through a random 2^4 sub-cube instead of inverting the key: all 4096 cells of the sub-cube, sorted, are one run.
    rng = np.random.default_rng(6)
    gx, gy, gz = _grid(4)
    for _ in range(20):
        base = rng.integers(0, 1 << 17, 3, dtype=np.uint32) << np.uint32(4)
        cx, cy, cz = gx + base[0], gy + base[1], gz + base[2]
        key = _keys(lib, HILBERT, 21, cx, cy, cz)
        order = np.argsort(key)
        assert np.array_equal(np.diff(key[order]), np.ones(len(key) - 1, np.uint64)), "an octree cell is not one run of keys"
        cells = np.stack([cx, cy, cz], 1).astype(np.int64)[order]
        assert np.all(np.abs(np.diff(cells, axis=0)).sum(1) == 1)


@pytest.mark.parametrize("curve", [HILBERT, MORTON])
def test_key_prefix_is_the_parent_cells_key(lib, curve):
    """The Karras prerequisite, for every m: key_L(cell) >> 3 (L - m) == key_m(cell >> (L - m))."""
    x, y, z = _random_cells(50_000, seed=7)
    key = _keys(lib, curve, 21, x, y, z)
    for m in range(1, 21):
        s = np.uint32(21 - m)
        assert np.array_equal(key >> np.uint64(3 * (21 - m)), _keys(lib, curve, m, x >> s, y >> s, z >> s)), m
    for levels in (3, 4):
        x, y, z = _grid(levels)
        key = _keys(lib, curve, levels, x, y, z)
        for m in range(1, levels):
            s = np.uint32(levels - m)
            assert np.array_equal(key >> np.uint64(3 * (levels - m)), _keys(lib, curve, m, x >> s, y >> s, z >> s))


@pytest.mark.parametrize("curve", [HILBERT, MORTON])
def test_point_key_quantisation_and_nan(lib, curve):
    rng = np.random.default_rng(8)
    xyz = (rng.random((5000, 3), dtype=np.float32) * np.float32(3.0) - np.float32(1.0)).astype(np.float32)
    lo, ext = xyz.min(0), np.float32((xyz.max(0) - xyz.min(0)).max())
    for levels, top in ((21, 2097151.0), (10, 1023.0)):
        scale = np.float32(top) / ext
        cells = np.clip((xyz - lo) * scale, np.float32(0), np.float32(top)).astype(np.uint32)
        want = (np_hilbert if curve == HILBERT else np_interleave)(cells[:, 0], cells[:, 1], cells[:, 2], levels)
        assert np.array_equal(_point_keys(lib, curve, levels, xyz, lo, ext), want)
    bad = xyz[:6].copy()
    for i in range(6):
        bad[i, i % 3] = np.nan
    bad[5, :] = np.nan
    assert np.all(_point_keys(lib, curve, 21, bad, lo, ext) == np.uint64(1) << np.uint64(63))
    assert np.all(_point_keys(lib, curve, 10, bad, lo, ext) == np.uint64(1) << np.uint64(30))
    # every real point sorts below them, also one outside the scene box (clamped to a face) and in a degenerate scene
    far = np.array([[1e30, -1e30, 0.5]], np.float32)
    assert _point_keys(lib, curve, 21, far, lo, ext)[0] < np.uint64(1) << np.uint64(63)
    assert np.all(_point_keys(lib, curve, 21, xyz[:10], lo, np.float32(0.0)) == 0)


# ---- the block-list model ----
def _blocks_per_query(pts, key, k, level, packets, seed):
    """Points sorted by `key` and cut into blocks of 16; a query needs a block if the block's box meets [q - r, q + r],
    r = 0.25 (k / n)^(1/3) 2^level; mean over the queries of `packets` random packets of 64 consecutive sorted points."""
    n = len(pts)
    p = pts[np.argsort(key, kind="stable")]
    blocks = p[: n // 16 * 16].reshape(-1, 16, 3)
    blo, bhi = blocks.min(1), blocks.max(1)
    r = np.float32(0.25 * (k / n) ** (1.0 / 3.0) * 2 ** level)
    counts = []
    for s in np.random.default_rng(seed).integers(0, n // 64 - 1, packets):
        q = p[s * 64:(s + 1) * 64]
        near = np.nonzero(np.all((blo <= q.max(0) + r) & (bhi >= q.min(0) - r), axis=1))[0]
        hit = np.all((blo[near][None] <= (q + r)[:, None]) & (bhi[near][None] >= (q - r)[:, None]), axis=2)
        counts.extend(hit.sum(1))
    return float(np.mean(counts))


def test_hilbert_order_shortens_the_block_lists(lib):
    """Measured with this model at n = 4e5, k = 10, 40 packets: 28.6 blocks per query at level 2 along the Z curve, 19.6
    along the Hilbert curve (0.69 x).  The bound 0.8 x leaves room for the sampling noise of 40 packets; a key that is a
    mere permutation of the Z curve's cells does not pass."""
    n, k = 400_000, 10
    pts = np.random.default_rng(0).random((n, 3), dtype=np.float32)
    lo, ext = pts.min(0), np.float32((pts.max(0) - pts.min(0)).max())
    per = {}
    for name, curve in (("morton", MORTON), ("hilbert", HILBERT)):
        key = _point_keys(lib, curve, 21, pts, lo, ext)
        per[name] = [_blocks_per_query(pts, key, k, level, packets=40, seed=1) for level in (1, 2)]
    print("blocks per query, level 1 / level 2: morton %.1f / %.1f, hilbert %.1f / %.1f" % (*per["morton"], *per["hilbert"]))
    assert per["hilbert"][1] < 0.8 * per["morton"][1]
    assert per["hilbert"][0] < 0.8 * per["morton"][0]
