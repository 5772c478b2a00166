"""What tknnVoxelGrid (include/owlknn_voxel.h) refuses, one fault per row and in the header's order, that the message names the call
and the field, and that a refused call writes nothing, neither outputs nor info."""
import ctypes

import numpy as np
import pytest

import voxel_spec as vs

pytestmark = pytest.mark.gpu

ARG = -1
TOO_MANY = 2 ** 31 - 1


def test_voxel_grid_error_codes_in_order():
    import torch

    from owlraytracing_amd import _voxel_lib as vl
    from owlraytracing_amd.trueknn import TrueKNN

    lib = vl.load()
    eng = TrueKNN(device=0)  # no tree
    dev = eng.device
    n, C, B, guard = 500, 3, 2, 64
    rng = np.random.default_rng(0)
    P, values = vs.uniform(n, 1), rng.random((n, C), dtype=np.float32)
    batch = (np.arange(n) % B).astype(np.int32)
    want = vs.grid(P, 0.25, (0, 0, 0), batch=batch, B=B, values=values)
    V = want["V"]
    d_points, d_values, d_batch = torch.from_numpy(P).to(dev), torch.from_numpy(values).to(dev), torch.from_numpy(batch).to(dev)
    widths = {"d_cell": 3, "d_count": 1, "d_centroid": 3, "d_value_mean": C, "d_first": 1, "d_nearest": 1, "d_voxel_label": 1}
    bufs = {name: torch.full(((n + guard) * w,), -7, dtype=torch.float32 if name in ("d_centroid", "d_value_mean") else torch.int32, device=dev)
            for name, w in widths.items()}
    bufs["d_offsets"] = torch.full((B + 1 + guard,), -7, dtype=torch.int64, device=dev)
    bufs["d_map"] = torch.full((n + guard,), -7, dtype=torch.int32, device=dev)
    info = vl.VoxelGridInfo()

    def call(handle=None, options=True, with_info=True, outputs=tuple(bufs), origin=(0.0, 0.0, 0.0), **kw):
        o = vl.VoxelGridOptions()
        o.n, o.d_points, o.d_values, o.d_batch = n, d_points.data_ptr(), d_values.data_ptr(), d_batch.data_ptr()
        o.voxel, o.num_batches, o.channels, o.capacity = 0.25, B, C, n
        for axis in range(3):
            o.origin[axis] = origin[axis]
        for name in outputs:
            setattr(o, name, bufs[name].data_ptr())
        for name, v in kw.items():
            setattr(o, name, v)
        info.voxels, info.max_count, info.solve_ms = 99, 98, 97.0
        rc = lib.tknnVoxelGrid(eng._h if handle is None else handle, ctypes.byref(o) if options else None, ctypes.byref(info) if with_info else None, None)
        torch.cuda.synchronize()
        assert rc == 0 or (info.voxels == 99 and info.max_count == 98 and info.solve_ms == 97.0), "a refused call leaves the info alone"
        return rc

    def untouched(but=()):
        return all(bool((b == -7).all()) for name, b in bufs.items() if name not in but)

    def text():
        t = lib.tknnLastError().decode()
        assert t.startswith("tknnVoxelGrid: "), t
        return t

    # 1. NULL engine, options, info -- before any value
    assert call(handle=ctypes.c_void_p()) == ARG and "engine" in text()
    assert call(options=False) == ARG and "options" in text()
    assert call(with_info=False) == ARG and "info" in text()
    assert call(with_info=False, d_points=None, voxel=0.0) == ARG and "info" in text()
    # 2. d_points NULL with n > 0
    assert call(d_points=None) == ARG and "d_points" in text()
    assert call(d_points=None, d_values=None, n=-1) == ARG and "d_points" not in text(), "n <= 0 needs no points"
    assert call(d_points=None, d_values=None) == ARG and "d_points" in text()
    # 3. the values' pointers
    assert call(d_values=None) == ARG and "d_values" in text()
    assert call(d_values=None, voxel=-1.0) == ARG and "d_values" in text()
    assert call(channels=0) == ARG and "d_value_mean" in text()
    assert call(channels=0, n=-1) == ARG and "d_value_mean" in text()
    # 4. the values, in the header's order
    for bad in (-1, TOO_MANY):
        assert call(n=bad) == ARG and "<= n <" in text()
        assert call(n=bad, voxel=0.0) == ARG and "<= n <" in text()
    for bad in (0.0, -0.25, float("inf"), float("nan")):
        assert call(voxel=bad) == ARG and "voxel" in text()
        assert call(voxel=bad, num_batches=0) == ARG and "voxel" in text()
    for axis in range(3):
        for bad in (float("inf"), float("-inf"), float("nan")):
            origin = [0.0, 0.0, 0.0]
            origin[axis] = bad
            assert call(origin=origin) == ARG and "origin" in text()
            assert call(origin=origin, num_batches=0) == ARG and "origin" in text()
    for bad in (0, -1, 32769):
        assert call(num_batches=bad) == ARG and "num_batches" in text()
        assert call(num_batches=bad, channels=17) == ARG and "num_batches" in text()
    assert call(d_batch=None) == ARG and "without d_batch" in text()
    for bad in (-1, 17):
        assert call(channels=bad, capacity=-1) == ARG and "channels" in text()
    for bad in (-1, TOO_MANY):
        assert call(capacity=bad) == ARG and "<= capacity <" in text()
        assert call(capacity=bad, flags=1) == ARG and "<= capacity <" in text()
    for bad in (1, 8, 0x80000000):
        assert call(flags=bad) == ARG and "flag" in text()
    # 5. more voxels than the capacity: found on the device, nothing written
    assert call(capacity=V - 1) == ARG and "capacity" in text() and str(V) in text()
    assert call(capacity=0) == ARG and "capacity" in text()
    assert untouched(), "a refused call writes nothing"
    # the count pass looks at no capacity beyond its range; n = 0 succeeds with V = 0, filled tails and offsets all 0
    assert call(outputs=("d_map", "d_offsets"), capacity=0) == 0 and info.voxels == V and untouched(but=("d_map", "d_offsets"))
    for b in bufs.values():
        b.fill_(-7)
    assert call(n=0, d_points=None, d_batch=None, num_batches=1, capacity=5) == 0
    assert (info.voxels, info.rows_in_grid, info.bad_rows, info.max_count) == (0, 0, 0, 0)
    assert bufs["d_offsets"][:2].tolist() == [0, 0] and (bufs["d_offsets"][2:] == -7).all() and (bufs["d_map"] == -7).all()
    assert (bufs["d_count"][:5] == 0).all() and (bufs["d_count"][5:] == -7).all() and (bufs["d_cell"][:15] == -1).all() and (bufs["d_cell"][15:] == -7).all()
    assert torch.isnan(bufs["d_centroid"][:15]).all() and (bufs["d_centroid"][15:] == -7).all() and torch.isnan(bufs["d_value_mean"][:5 * C]).all()
    assert (bufs["d_first"][:5] == -1).all() and (bufs["d_nearest"][:5] == -1).all() and (bufs["d_voxel_label"][:5] == -1).all()
    # the call itself: nothing is written behind the capacity, the offsets or the rows
    for b in bufs.values():
        b.fill_(-7)
    assert call() == 0 and info.voxels == V and info.rows_in_grid == n and info.solve_ms > 0 and info.sort_ms > 0 and info.key_ms > 0 and info.reduce_ms > 0
    assert np.array_equal(bufs["d_count"][:V].cpu().numpy(), want["counts"]) and np.array_equal(bufs["d_map"][:n].cpu().numpy(), want["map"])
    assert np.array_equal(bufs["d_offsets"][:B + 1].cpu().numpy(), want["offsets"])
    for name, w in widths.items():
        assert (bufs[name][n * w:] == -7).all(), name
    assert (bufs["d_offsets"][B + 1:] == -7).all() and (bufs["d_map"][n:] == -7).all()
    eng.close()
