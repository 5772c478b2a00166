"""Host side of the TrueKNN engine above the C-ABI (include/owlknn.h).

Mirrors what ``samples/s01-trueknn/hostCode.cpp`` does with its command line
``file n dim start_radius k timefile``: upload points, build the accel (hostCode.cpp:201-206),
run the radius-doubling solve (hostCode.cpp:285-340) and expose the frameBuffer rows.
torch is used only to own device memory and the stream.
"""
import ctypes

import numpy as np

from . import (_batch_lib, _emst_lib, _fpfh_lib, _fps_lib, _global_lib, _hdbscan_lib, _icp_lib, _knn_lib, _lib, _meanshift_lib, _nms_lib, _orient_lib, _pca_lib, _periodic_lib,
               _plane_lib, _reduce_lib, _voxel_lib)
from .datasets import pad_to_3d

NEIGH_BYTES = 24  # GeomTypes.h:22-28


def _call_outputs(torch, device, wanted):
    """The outputs of one tknnVoxelGrid, tknnOrientNormals or tknnSegmentPlane call: {name: an uninitialised tensor} for ``wanted`` = {name: (shape,
    dtype)}, and "spare", the address an empty one stands for.  ``torch`` is the engine's handle (TrueKNN._torch), so what stands in
    for it in the tests -- tests/guarded_outputs.py -- sees every one of them (tests/test_voxel_gpu.py and tests/test_orient_gpu.py
    run the wrappers under it)."""
    out = {name: torch.empty(shape, dtype=dtype, device=device) for name, (shape, dtype) in wanted.items()}
    spare = torch.empty((4,), dtype=torch.int32, device=device)
    out["spare"] = spare
    return out


def _address(t, spare=None):
    """What a call is given for the optional tensor ``t``: NULL for None, its address, or -- an empty tensor has no
    address -- that of ``spare`` (with m = 0 a query call is a no-op that still checks its arguments)."""
    if t is None:
        return None
    return t.data_ptr() if t.numel() > 0 else _address(spare)


class TrueKNN:
    """One engine on one GPU.  ``points`` may be a numpy array (n,2|3) or a CUDA float32 tensor (n,3)."""

    def __init__(self, device=None):
        import torch

        self._torch = torch
        lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("TrueKNN needs an MI355X: no GPU is visible and there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self._lib = lib
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.tknnCreate(ctypes.byref(self._h)))
        self.n = 0
        self.halo_n = 0
        self.num_clouds = 1  # the batches of a batched tree (fps samples each), 1 for a plain one
        self._row_names = None
        self.build_info = None
        self.last_info = None

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.tknnDestroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _points(self, points):
        torch = self._torch
        if isinstance(points, np.ndarray):
            points = torch.from_numpy(pad_to_3d(points)).to(self.device)
        if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or not points.is_cuda:
            raise ValueError("points must be float32 (n,3) on the GPU")
        return points.contiguous()

    def _ids(self, ids, n):
        torch = self._torch
        if ids is None:
            return None
        if isinstance(ids, np.ndarray):
            ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(self.device)
        if ids.dtype != torch.int32 or ids.dim() != 1 or ids.shape[0] != n or not ids.is_cuda:
            raise ValueError("ids must be int32 (n,) on the GPU")
        return ids.contiguous()

    def _queries(self, queries, who):
        """The ``queries`` of the query call ``who`` as the library takes them: a contiguous float32 (m,3) tensor on the
        engine's device; a numpy array (m,2|3) is padded and uploaded."""
        torch = self._torch
        if isinstance(queries, np.ndarray):
            if queries.ndim != 2 or queries.shape[1] not in (2, 3):
                raise ValueError("%s: queries must be (m,2) or (m,3), got %s" % (who, queries.shape))
            queries = torch.from_numpy(pad_to_3d(queries)).to(self.device)
        if not isinstance(queries, torch.Tensor):
            raise ValueError("%s: queries must be a numpy array or a torch tensor" % who)
        if queries.dtype != torch.float32 or queries.dim() != 2 or queries.shape[1] != 3:
            raise ValueError("%s: queries must be float32 (m,3), got %s %s" % (who, queries.dtype, tuple(queries.shape)))
        if queries.device != self.device:
            raise ValueError("%s: queries are on %s, the engine on %s" % (who, queries.device, self.device))
        if not queries.is_contiguous():
            raise ValueError("%s: queries must be contiguous (packed fp32 triples)" % who)
        return queries

    def _written_in_place(self, who, what, t, shape, dtype):
        """``t`` (``what`` in the messages of ``who``) is a contiguous tensor of that shape and dtype on the engine's device:
        the library writes it through its address."""
        torch = self._torch
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s must be a tensor" % (who, what))
        if tuple(t.shape) != shape or t.dtype != dtype:
            raise ValueError("%s: %s must be %s %s, got %s %s" % (who, what, dtype, shape, t.dtype, tuple(t.shape)))
        if t.device != self.device:
            raise ValueError("%s: %s is on %s, the engine on %s" % (who, what, t.device, self.device))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous (it is written in place)" % (who, what))

    def build(self, points, ids=None, batch=None, num_batches=None):
        """LBVH over the points.  ``ids`` (optional int32) are the identities reported in neighbour
        lists (global indices when these points are one tile of a larger set).
        ``batch`` (optional, (n,) int32 labels, numpy or a tensor on the engine's device, in any order): the points are
        ``num_batches`` clouds in one tree (tknnBuildBatched) -- every call treats the tree as one set but ``batch_knn``,
        which looks for neighbours inside a query's own cloud.  ``num_batches`` defaults to the largest label + 1."""
        torch = self._torch
        points = self._points(points)
        ids = self._ids(ids, points.shape[0])
        info = _lib.BuildInfo()
        if batch is None:
            if num_batches is not None:
                raise ValueError("build: num_batches goes with batch")
            with torch.cuda.device(self.device):
                _lib.check(self._lib.tknnBuildIds(self._h, ctypes.c_void_p(points.data_ptr()),
                                                  None if ids is None else ctypes.c_void_p(ids.data_ptr()),
                                                  points.shape[0], ctypes.byref(info), self._stream()))
        else:
            with torch.cuda.device(self.device):
                batch = self._labels(batch, points.shape[0], "build", "batch", "point")
                if num_batches is None:
                    num_batches = int(batch.max()) + 1  # (a negative label is refused by the library)
                _lib.check(_batch_lib.load().tknnBuildBatched(self._h, ctypes.c_void_p(points.data_ptr()),
                                                              None if ids is None else ctypes.c_void_p(ids.data_ptr()),
                                                              ctypes.c_void_p(batch.data_ptr()), int(num_batches), points.shape[0],
                                                              ctypes.byref(info), self._stream()))
        self.n = int(points.shape[0])
        self.num_clouds = 1 if batch is None else int(num_batches)
        self._row_names = ids  # the names of the rows (radius_nms turns kept rows into names), None: the rows themselves
        self.halo_n = 0  # a build drops the halo tree
        self.build_info = info.as_dict()
        return self.build_info

    def _labels(self, values, count, who, name, per):
        """Batch labels as the library takes them: a contiguous int32 (count,) tensor on the engine's device."""
        torch = self._torch
        if isinstance(values, torch.Tensor) and values.device != self.device:
            raise ValueError("%s: %s is on %s, the engine on %s" % (who, name, values.device, self.device))
        values = torch.as_tensor(values, device=self.device).to(torch.int32).contiguous()
        if values.shape != (count,):
            raise ValueError("%s: %s must have one entry per %s" % (who, name, per))
        return values

    def batch_layout(self):
        """What the last batched ``build`` made (tknnBatchLayout): dict(num_batches, key_bits, starts) -- ``starts`` a
        (num_batches + 1,) int32 tensor on the engine's device, batch b being the sorted slots starts[b] .. starts[b + 1] - 1
        of the tree and starts[num_batches] the number of points without a NaN."""
        torch = self._torch
        lib = _batch_lib.load()
        nb, bits = ctypes.c_int32(0), ctypes.c_int32(0)
        with torch.cuda.device(self.device):
            _lib.check(lib.tknnBatchLayout(self._h, ctypes.byref(nb), ctypes.byref(bits), None, self._stream()))
            starts = torch.empty((nb.value + 1,), dtype=torch.int32, device=self.device)
            _lib.check(lib.tknnBatchLayout(self._h, None, None, ctypes.c_void_p(starts.data_ptr()), self._stream()))
        return {"num_batches": int(nb.value), "key_bits": int(bits.value), "starts": starts}

    def set_halo(self, points=None, ids=None):
        """Second point set every query also searches (border points of neighbouring tiles)."""
        torch = self._torch
        with torch.cuda.device(self.device):
            if points is None or len(points) == 0:
                _lib.check(self._lib.tknnSetHalo(self._h, None, None, 0, self._stream()))
                self.halo_n = 0
                return
            points = self._points(points)
            ids = self._ids(ids, points.shape[0])
            if ids is None:
                raise ValueError("halo points need ids")
            _lib.check(self._lib.tknnSetHalo(self._h, ctypes.c_void_p(points.data_ptr()),
                                             ctypes.c_void_p(ids.data_ptr()), points.shape[0], self._stream()))
            torch.cuda.current_stream(self.device).synchronize()  # the engine copied what it needs
            self.halo_n = int(points.shape[0])

    def halo_select(self, boxes, box_peer, npeers):
        """Send side of the halo exchange: my points inside any of ``boxes`` (m,6 float32 closed boxes,
        lo xyz hi xyz) of each peer ``box_peer[j]``.  Returns (rows, counts): rows (sum(counts), 4)
        float32 wire rows x y z id-bits with peer p's rows contiguous (in peer order), counts a
        python list of length npeers.  Row order inside a peer's segment is unspecified."""
        torch = self._torch
        with torch.cuda.device(self.device):
            dev = self.device
            boxes = torch.as_tensor(boxes, dtype=torch.float32, device=dev).contiguous().view(-1, 6)
            box_peer = torch.as_tensor(box_peer, dtype=torch.int32, device=dev).contiguous()
            counts = torch.empty(npeers, dtype=torch.int64, device=dev)
            args = (self._h, ctypes.c_void_p(boxes.data_ptr()), ctypes.c_void_p(box_peer.data_ptr()), int(len(box_peer)), int(npeers))
            _lib.check(self._lib.tknnHaloSelect(*args, ctypes.c_void_p(counts.data_ptr()), None, None, self._stream()))
            host_counts = counts.cpu()  # the caller needs them on the host anyway (message sizes)
            offsets = (torch.cumsum(host_counts, 0) - host_counts).to(dev)
            total = int(host_counts.sum())
            rows = torch.empty((total, 4), dtype=torch.float32, device=dev)
            if total:
                _lib.check(self._lib.tknnHaloSelect(*args, None, ctypes.c_void_p(offsets.data_ptr()),
                                                    ctypes.c_void_p(rows.data_ptr()), self._stream()))
            return rows, host_counts.tolist()

    def halo_select_fixed(self, boxes, box_peer, npeers, caps):
        """The one-pass form of ``halo_select`` for the fixed-capacity exchange (tknnHaloSelectFixed): ``caps[p]`` rows per peer.
        Returns (messages, starts, counts): ``messages`` a (sum(caps) + npeers, 4) float32 buffer in which peer p's message is
        rows starts[p] .. starts[p] + caps[p] -- a header row (the count, as two float32 cells that hold integers below 2**24
        exactly) and caps[p] wire rows, those past the count left untouched (``messages`` is not initialised) --, ``counts`` the exact per-peer counts as an int64
        DEVICE tensor (a count above its capacity: rows were dropped, the caller falls back to ``halo_select``).  Nothing in
        here waits for the device."""
        torch = self._torch
        with torch.cuda.device(self.device):
            dev = self.device
            boxes = torch.as_tensor(boxes, dtype=torch.float32, device=dev).contiguous().view(-1, 6)
            box_peer = torch.as_tensor(box_peer, dtype=torch.int32, device=dev).contiguous()
            caps = [int(c) for c in caps]
            starts, at = [], 0
            for c in caps:
                starts.append(at)
                at += c + 1
            messages = torch.empty((at, 4), dtype=torch.float32, device=dev)
            caps_dev = torch.tensor(caps, dtype=torch.int64, device=dev)
            offsets = torch.tensor([s0 + 1 for s0 in starts], dtype=torch.int64, device=dev)
            counts = torch.empty(npeers, dtype=torch.int64, device=dev)
            _lib.check(self._lib.tknnHaloSelectFixed(self._h, ctypes.c_void_p(boxes.data_ptr()), ctypes.c_void_p(box_peer.data_ptr()), int(len(box_peer)),
                                                     int(npeers), ctypes.c_void_p(caps_dev.data_ptr()), ctypes.c_void_p(offsets.data_ptr()),
                                                     ctypes.c_void_p(messages.data_ptr()), ctypes.c_void_p(counts.data_ptr()), self._stream()))
            heads = torch.tensor(starts, dtype=torch.int64, device=dev)
            # (the header cells distributed._count_cells writes on the host; distributed._count_of_cells reads them)
            messages[heads, 0] = (counts % (1 << 24)).float()
            messages[heads, 1] = (counts >> 24).float()
            return messages, starts, counts

    supports_phases = True  # solve(phase=1 | 2): interior / boundary queries of a tile (tknnSolveOptions.phase)

    def solve(self, k, start_radius, kernel=_lib.KERNEL_AUTO, max_rounds=64, want_fb=False,
              out=None, want_levels=False, allow_unfinished=False, phase=0, stream=None, start_radii=None, fb_only=False):
        """Returns dict(idx (n,k) int32, dist (n,k) f32, intersections (n,) int64[, fb (n*k*24,) uint8])
        as CUDA tensors plus ``info``.  ``out`` may carry preallocated tensors of those names.
        ``phase`` 1 / 2: only the interior / boundary queries marked by the last ``halo_select`` (sharded use);
        ``stream``: a torch.cuda.Stream to launch on instead of the current one (a phase-1 solve runs on a
        stream and host thread of its own beside the halo exchange).
        ``start_radii``: (n,) float32, a start radius per query (row) instead of ``start_radius`` for all -- the opt-in
        per-query radius schedule (tknnSolveOptions.d_start_radii).
        ``fb_only``: only the reference's frameBuffer records are written (d_idx = d_dist = d_intersections = NULL), the
        way the reference's own host code receives its results."""
        torch = self._torch
        n = self.n
        out = dict(out or {})
        with torch.cuda.device(self.device):
            if n > 0 and k > 0:
                if not fb_only:
                    out.setdefault("idx", torch.empty((n, k), dtype=torch.int32, device=self.device))
                    out.setdefault("dist", torch.empty((n, k), dtype=torch.float32, device=self.device))
                    out.setdefault("intersections", torch.empty((n,), dtype=torch.int64, device=self.device))
                if want_fb or fb_only:
                    out.setdefault("fb", torch.empty((n * k * NEIGH_BYTES,), dtype=torch.uint8, device=self.device))
                if want_levels or allow_unfinished:
                    out.setdefault("levels", torch.empty((n,), dtype=torch.int32, device=self.device))
            info = _lib.SolveInfo()

            def ptr(name):
                t = out.get(name)
                return ctypes.c_void_p(t.data_ptr()) if t is not None else None

            opt = _lib.SolveOptions()
            opt.k, opt.start_radius, opt.kernel = int(k), float(start_radius), int(kernel)
            opt.max_rounds, opt.allow_unfinished = int(max_rounds), int(bool(allow_unfinished))
            opt.phase = int(phase)
            radii = None
            if start_radii is not None:
                radii = torch.as_tensor(start_radii, dtype=torch.float32, device=self.device).contiguous()
                if radii.shape != (n,):
                    raise ValueError("start_radii must have one entry per point")
                opt.d_start_radii = radii.data_ptr()
            for field, name in (("d_idx", "idx"), ("d_dist", "dist"), ("d_intersections", "intersections"),
                                ("d_fb", "fb"), ("d_levels", "levels")):
                p = ptr(name)
                setattr(opt, field, p.value if p is not None else None)
            launch_on = self._stream() if stream is None else ctypes.c_void_p(stream.cuda_stream)
            _lib.check(self._lib.tknnSolveEx(self._h, ctypes.byref(opt), ctypes.byref(info), launch_on))
        self.last_info = info.as_dict()
        out["info"] = self.last_info
        return out

    def repair_exact(self, result, k, start_radius):
        """Turn the finished rows of ``solve(..., want_levels=True)`` into exact kNN in (dist, index) order, in place (opt-in;
        the reference's box-candidate rows are what ``solve`` returns).  Returns the number of rows whose contents changed.
        ``result`` must hold contiguous ``idx`` (n,k) int32, ``dist`` (n,k) float32 and ``levels`` (n,) int32 on the
        engine's device: the pass writes n*k entries through their pointers."""
        torch = self._torch
        n, k = self.n, int(k)
        if "levels" not in result or result["levels"] is None:
            raise ValueError("repair_exact needs the levels of the solve (solve(..., want_levels=True))")
        for name, shape, dtype in (("idx", (n, k), torch.int32), ("dist", (n, k), torch.float32), ("levels", (n,), torch.int32)):
            self._written_in_place("repair_exact", "result[%r]" % name, result.get(name), shape, dtype)
        n_fixed = ctypes.c_int64(0)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.tknnRepairExact(
                self._h, int(k), ctypes.c_float(start_radius), ctypes.c_void_p(result["levels"].data_ptr()),
                ctypes.c_void_p(result["idx"].data_ptr()), ctypes.c_void_p(result["dist"].data_ptr()),
                ctypes.byref(n_fixed), self._stream()))
        return int(n_fixed.value)

    def query(self, queries, k, start_radius, max_rounds=64, exact=False, allow_unfinished=False, want_levels=False,
              out=None, stream=None):
        """TrueKNN rows for points that are NOT in the built set (tknnQuery): row j is what the reference's loop gives
        q_j in the set P + {q_j}; a point of P at distance 0 is an ordinary neighbour.  ``queries``: numpy (m,2|3) or a
        contiguous float32 CUDA tensor (m,3) on the engine's device.  Returns dict(idx (m,k) int32, dist (m,k) float32,
        intersections (m,) int64[, levels (m,) int32], info).  ``exact``: rows rewritten as the true k nearest points
        in (dist, index) order.  ``out`` may carry preallocated contiguous tensors of those names."""
        torch = self._torch
        k = int(k)
        queries = self._queries(queries, "query")
        m = int(queries.shape[0])
        out = dict(out or {})
        shapes = {"idx": ((m, k), torch.int32), "dist": ((m, k), torch.float32), "intersections": ((m,), torch.int64),
                  "levels": ((m,), torch.int32)}
        for name, t in out.items():
            if name not in shapes:
                raise ValueError("query: out[%r] is not an output of query" % name)
            self._written_in_place("query", "out[%r]" % name, t, *shapes[name])
        with torch.cuda.device(self.device):
            names = ["idx", "dist", "intersections"] + (["levels"] if want_levels or allow_unfinished else [])
            for name in names:
                if name not in out:
                    shape, dtype = shapes[name]
                    out[name] = torch.empty(tuple(max(d, 0) for d in shape), dtype=dtype, device=self.device)
            opt = _lib.QueryOptions()
            opt.m, opt.k, opt.start_radius = m, k, float(start_radius)
            opt.max_rounds, opt.allow_unfinished, opt.exact = int(max_rounds), int(bool(allow_unfinished)), int(bool(exact))
            spare = torch.empty((1,), dtype=torch.int64, device=self.device) if m == 0 else None
            opt.d_queries = _address(queries)
            for field, name in (("d_idx", "idx"), ("d_dist", "dist"), ("d_intersections", "intersections"), ("d_levels", "levels")):
                setattr(opt, field, _address(out.get(name), spare))
            info = _lib.SolveInfo()
            launch_on = self._stream() if stream is None else ctypes.c_void_p(stream.cuda_stream)
            _lib.check(self._lib.tknnQuery(self._h, ctypes.byref(opt), ctypes.byref(info), launch_on))
        self.last_info = info.as_dict()
        out["info"] = self.last_info
        return out

    def dbscan(self, eps, min_pts, want_counts=False):
        """RT-DBSCAN over the built tree: dict(labels int32 (n,), core bool (n,), [counts], info)."""
        torch = self._torch
        n = self.n
        with torch.cuda.device(self.device):
            labels = torch.empty((n,), dtype=torch.int32, device=self.device)
            core = torch.empty((n,), dtype=torch.uint8, device=self.device)
            counts = torch.empty((n,), dtype=torch.int32, device=self.device) if want_counts else None
            info = _lib.DbscanInfo()
            _lib.check(self._lib.tknnDbscan(self._h, ctypes.c_float(eps), int(min_pts), ctypes.c_void_p(labels.data_ptr()),
                                            ctypes.c_void_p(core.data_ptr()),
                                            None if counts is None else ctypes.c_void_p(counts.data_ptr()),
                                            ctypes.byref(info), self._stream()))
        out = {"labels": labels, "core": core.view(torch.bool), "info": info.as_dict()}
        if counts is not None:
            out["counts"] = counts
        return out

    def dbscan_auto(self, eps0, min_pts, max_noise=0.05, max_rounds=32):
        """RT-DBSCAN with an auto-grown eps (tknnDbscanAuto): eps doubles from ``eps0`` until at most
        floor(max_noise * n) points are noise.  dict(labels, core, info(rounds, eps, noise, clusters, ...))."""
        torch = self._torch
        n = self.n
        with torch.cuda.device(self.device):
            labels = torch.empty((n,), dtype=torch.int32, device=self.device)
            core = torch.empty((n,), dtype=torch.uint8, device=self.device)
            info = _lib.DbscanAutoInfo()
            _lib.check(self._lib.tknnDbscanAuto(self._h, ctypes.c_float(eps0), int(min_pts), ctypes.c_double(max_noise), int(max_rounds),
                                                ctypes.c_void_p(labels.data_ptr()), ctypes.c_void_p(core.data_ptr()),
                                                ctypes.byref(info), self._stream()))
        return {"labels": labels, "core": core.view(torch.bool), "info": info.as_dict()}

    def dbscan_noise(self, eps, min_pts):
        """Which points tknnDbscan(eps, min_pts) would label -1, without building clusters (tknnDbscanNoise: one growth
        round of the auto-eps loop for a caller that runs the loop itself).  dict(noise (n,) bool, count)."""
        torch = self._torch
        with torch.cuda.device(self.device):
            noise = torch.empty((self.n,), dtype=torch.uint8, device=self.device)
            count = ctypes.c_int64(0)
            _lib.check(self._lib.tknnDbscanNoise(self._h, ctypes.c_float(eps), int(min_pts), ctypes.c_void_p(noise.data_ptr()),
                                                 ctypes.byref(count), self._stream()))
        return {"noise": noise.view(torch.bool), "count": int(count.value)}

    def dbscan_assign(self, eps, core_label):
        """Last step of DBSCAN with labels decided by the caller: ``core_label`` (n,) int32, >= 0 for
        core points.  Returns labels (n,) int32: core points keep theirs, the others take the smallest
        label among the core points within eps, -1 if there is none."""
        torch = self._torch
        with torch.cuda.device(self.device):
            core_label = torch.as_tensor(core_label, dtype=torch.int32, device=self.device).contiguous()
            if core_label.shape != (self.n,):
                raise ValueError("core_label must have one entry per point")
            labels = torch.empty((self.n,), dtype=torch.int32, device=self.device)
            info = _lib.DbscanInfo()
            _lib.check(self._lib.tknnDbscanAssign(self._h, ctypes.c_float(eps), ctypes.c_void_p(core_label.data_ptr()),
                                                  ctypes.c_void_p(labels.data_ptr()), ctypes.byref(info), self._stream()))
        return labels

    def dbscan_query(self, queries, eps, labels, core=None, want_counts=False):
        """Cluster labels for points that are NOT in the built set (tknnDbscanQuery): labels[j] is the smallest label among
        the core points of the set within ``eps`` of q_j, -1 if there is none; counts[j] the number of points of the set
        within ``eps`` (nothing is "self": a point of the set that coincides with q_j counts).  ``queries``: numpy (m,2|3) or
        a contiguous float32 CUDA tensor (m,3) on the engine's device.  ``labels`` (n,) int32 by row, with ``core`` (n,) bool
        the labels and core flags of a clustering (``dbscan``'s); without ``core`` it is the core-label array itself (>= 0:
        core with that label, < 0: not core, as ``dbscan_assign`` takes it).
        Returns dict(labels (m,) int32, [counts (m,) int32], info)."""
        torch = self._torch
        queries = self._queries(queries, "dbscan_query")
        m = int(queries.shape[0])
        with torch.cuda.device(self.device):
            core_label = torch.as_tensor(labels, dtype=torch.int32, device=self.device)
            if core_label.shape != (self.n,):
                raise ValueError("dbscan_query: labels must have one entry per point of the built set")
            if core is not None:
                core = torch.as_tensor(core, device=self.device).to(torch.bool)
                if core.shape != (self.n,):
                    raise ValueError("dbscan_query: core must have one entry per point of the built set")
                core_label = torch.where(core, core_label, torch.full_like(core_label, -1))
            core_label = core_label.contiguous()
            out = {"labels": torch.empty((m,), dtype=torch.int32, device=self.device)}
            if want_counts:
                out["counts"] = torch.empty((m,), dtype=torch.int32, device=self.device)
            spare = torch.empty((1,), dtype=torch.int32, device=self.device) if m == 0 else None
            opt = _lib.DbscanQueryOptions()
            opt.m, opt.eps = m, float(eps)
            opt.d_queries = _address(queries)
            opt.d_core_label = _address(core_label)
            opt.d_labels = _address(out["labels"], spare)
            opt.d_counts = _address(out.get("counts"), spare)
            info = _lib.DbscanInfo()
            _lib.check(self._lib.tknnDbscanQuery(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        out["info"] = info.as_dict()
        return out

    def radius_query(self, queries, radius, sort=True, want_dist=True):
        """The points of the built set within ``radius`` of each query, as CSR rows (tknnRadiusQuery): row j, the entries
        offsets[j] .. offsets[j + 1] of ``idx`` and ``dist``, holds the points p with the fp32 distance
        sqrt((dx*dx + dy*dy) + dz*dz) <= radius -- ``dbscan_query``'s predicate; nothing is "self".  ``queries``: numpy (m,2|3)
        or a contiguous float32 CUDA tensor (m,3) on the engine's device.  ``sort``: every row ascending in (distance, index);
        without it the order inside a row is unspecified.  The count pass sizes ``idx`` and ``dist``, the fill pass writes them.
        Returns dict(offsets (m+1,) int64, idx (total,) int32, dist (total,) float32 [with ``want_dist``], info); ``info`` is
        the fill pass's (the count pass's where there is nothing to fill), ``count_info`` the count pass's."""
        torch = self._torch
        queries = self._queries(queries, "radius_query")
        m = int(queries.shape[0])
        with torch.cuda.device(self.device):
            offsets = torch.empty((m + 1,), dtype=torch.int64, device=self.device)
            opt = _lib.RadiusOptions()
            opt.m, opt.radius, opt.sort = m, float(radius), int(bool(sort))
            opt.d_queries = _address(queries)
            opt.d_offsets = offsets.data_ptr()
            count_info = _lib.RadiusInfo()
            _lib.check(self._lib.tknnRadiusQuery(self._h, ctypes.byref(opt), ctypes.byref(count_info), self._stream()))
            total = int(count_info.total)
            out = {"offsets": offsets, "idx": torch.empty((total,), dtype=torch.int32, device=self.device)}
            if want_dist:
                out["dist"] = torch.empty((total,), dtype=torch.float32, device=self.device)
            info = count_info
            if total > 0:  # (an empty tensor has no address, and a NULL d_idx would ask for the count pass again)
                opt.d_idx, opt.capacity = out["idx"].data_ptr(), total
                opt.d_dist = out["dist"].data_ptr() if want_dist else None
                info = _lib.RadiusInfo()
                _lib.check(self._lib.tknnRadiusQuery(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        out["info"] = info.as_dict()
        out["count_info"] = count_info.as_dict()
        return out

    def radius_knn(self, queries, k, radius=None, radii=None, skip_ids=None, want_dist=True):
        """At most ``k`` nearest points of the built set within a radius of each query, as dense rows (tknnRadiusKnn): row j is
        the first min(k, len) entries of ``radius_query``'s sorted row at its radius -- the points p with the fp32 distance
        sqrt((dx*dx + dy*dy) + dz*dz) <= r_j, ascending in (distance, index) --, padded with idx -1 / dist +inf.  Exactly one of
        ``radius`` (one for all rows) and ``radii`` (length m, row j uses radii[j]; a row whose radius is NaN, not finite or <= 0
        is empty) is given.  ``skip_ids`` (length m, int32): the point named skip_ids[j] (its id on trees built with ids, its
        row otherwise) is left out of row j; a negative value skips nothing.  ``radii`` and ``skip_ids`` may be numpy arrays or
        tensors on the engine's device.  ``queries``: numpy (m,2|3) or a contiguous float32 CUDA tensor (m,3) on the engine's
        device.  Returns dict(idx (m,k) int32, dist (m,k) float32 [with ``want_dist``], counts (m,) int32, info)."""
        torch = self._torch
        queries = self._queries(queries, "radius_knn")
        if (radius is None) == (radii is None):
            raise ValueError("radius_knn: give exactly one of radius and radii")
        m, k = int(queries.shape[0]), int(k)

        def column(values, dtype, name):
            if isinstance(values, torch.Tensor) and values.device != self.device:
                raise ValueError("radius_knn: %s is on %s, the engine on %s" % (name, values.device, self.device))
            values = torch.as_tensor(values, device=self.device).to(dtype).contiguous()
            if values.shape != (m,):
                raise ValueError("radius_knn: %s must have one entry per query" % name)
            return values

        with torch.cuda.device(self.device):
            radii = None if radii is None else column(radii, torch.float32, "radii")
            skip_ids = None if skip_ids is None else column(skip_ids, torch.int32, "skip_ids")
            rows = max(k, 0)
            out = {"idx": torch.empty((m, rows), dtype=torch.int32, device=self.device)}
            if want_dist:
                out["dist"] = torch.empty((m, rows), dtype=torch.float32, device=self.device)
            out["counts"] = torch.empty((m,), dtype=torch.int32, device=self.device)
            spare = torch.empty((1,), dtype=torch.int32, device=self.device)
            opt = _lib.RadiusKnnOptions()
            opt.m, opt.k, opt.radius = m, k, 0.0 if radius is None else float(radius)
            opt.d_queries = _address(queries)
            opt.d_radii = _address(radii, spare)
            opt.d_skip_ids = _address(skip_ids)
            opt.d_idx = _address(out["idx"], spare)
            opt.d_dist = _address(out.get("dist"))
            opt.d_counts = _address(out["counts"])
            info = _lib.RadiusKnnInfo()
            _lib.check(self._lib.tknnRadiusKnn(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        out["info"] = info.as_dict()
        return out

    def knn(self, queries=None, k=1, skip_ids=None, want_dist=True):
        """The ``k`` nearest points of the built set, exactly and with no radius to choose, as dense rows (tknnKnn): row j holds
        the points p whose fp32 distance sqrt((dx*dx + dy*dy) + dz*dz) is finite, ascending in (distance, index), cut after k and
        padded with idx -1 / dist +inf -- ``radius_knn``'s row at the largest finite radius.  With ``queries`` (numpy (m,2|3) or
        a contiguous float32 CUDA tensor (m,3) on the engine's device) nothing is self unless ``skip_ids`` (length m, int32,
        numpy or a tensor on the engine's device) says so: the point named skip_ids[j] (its id on trees built with ids, its row
        otherwise) is left out of row j; a negative value skips nothing.  Without ``queries`` row j answers for point j of the
        built set, every point left out of its own row (a coinciding duplicate stays, at distance 0): the exact all-kNN of the
        set; ``skip_ids`` must then be None.  Returns dict(idx (m,k) int32, dist (m,k) float32 [with ``want_dist``], counts (m,)
        int32, info)."""
        torch = self._torch
        if queries is None:
            if skip_ids is not None:
                raise ValueError("knn: skip_ids go with queries (without queries every point is left out of its own row)")
            m = self.n
        else:
            queries = self._queries(queries, "knn")
            m = int(queries.shape[0])
        k = int(k)
        with torch.cuda.device(self.device):
            if skip_ids is not None:
                if isinstance(skip_ids, torch.Tensor) and skip_ids.device != self.device:
                    raise ValueError("knn: skip_ids is on %s, the engine on %s" % (skip_ids.device, self.device))
                skip_ids = torch.as_tensor(skip_ids, device=self.device).to(torch.int32).contiguous()
                if skip_ids.shape != (m,):
                    raise ValueError("knn: skip_ids must have one entry per query")
            rows = max(k, 0)
            out = {"idx": torch.empty((m, rows), dtype=torch.int32, device=self.device)}
            if want_dist:
                out["dist"] = torch.empty((m, rows), dtype=torch.float32, device=self.device)
            out["counts"] = torch.empty((m,), dtype=torch.int32, device=self.device)
            spare = torch.empty((1,), dtype=torch.int32, device=self.device)
            opt = _knn_lib.KnnOptions()
            opt.m, opt.k = m, k
            opt.d_queries = None if queries is None else _address(queries, spare)
            opt.d_skip_ids = _address(skip_ids, spare)
            opt.d_idx = _address(out["idx"], spare)
            opt.d_dist = _address(out.get("dist"))
            opt.d_counts = _address(out["counts"])
            info = _knn_lib.KnnInfo()
            _lib.check(_knn_lib.load().tknnKnn(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        out["info"] = info.as_dict()
        return out

    def emst(self, core_dist=None, want_components=False, max_rounds=0):
        """The minimum spanning forest of the built set (tknnEmst): Euclidean, or with ``core_dist`` ((n,) float32 by row, numpy or
        a contiguous tensor on the engine's device) under the mutual-reachability distance max(d, core[i], core[j]).  Edges are
        ordered by (bits of the fp32 weight, smaller name, larger name) -- names are ids on trees built with ids, rows otherwise
        --, which makes the forest unique; a point with a NaN coordinate, or whose core distance is not finite and >= 0, is in
        no edge.  Returns dict(u, v (edges,) int32 with u < v, w (edges,) float32, ascending by that key, edges, info[,
        components (n,) int32: the smallest row of the point's component, -1 for a point left out]).  ``max_rounds`` > 0 ends the
        Boruvka rounds early with TknnError (TKNN_E_ROUNDS); the default, and the most that is taken, is ceil(log2 n) + 1."""
        torch = self._torch
        n = self.n
        with torch.cuda.device(self.device):
            if core_dist is not None:
                if isinstance(core_dist, np.ndarray):
                    core_dist = torch.from_numpy(np.ascontiguousarray(core_dist, dtype=np.float32)).to(self.device)
                if not isinstance(core_dist, torch.Tensor):
                    raise ValueError("emst: core_dist must be a numpy array or a torch tensor")
                if core_dist.dtype != torch.float32 or tuple(core_dist.shape) != (n,):
                    raise ValueError("emst: core_dist must be float32 (n,), got %s %s" % (core_dist.dtype, tuple(core_dist.shape)))
                if core_dist.device != self.device:
                    raise ValueError("emst: core_dist is on %s, the engine on %s" % (core_dist.device, self.device))
                if not core_dist.is_contiguous():
                    raise ValueError("emst: core_dist must be contiguous")
            rows = max(n - 1, 0)
            u = torch.empty((rows,), dtype=torch.int32, device=self.device)
            v = torch.empty((rows,), dtype=torch.int32, device=self.device)
            w = torch.empty((rows,), dtype=torch.float32, device=self.device)
            comp = torch.empty((n,), dtype=torch.int32, device=self.device) if want_components else None
            spare = torch.empty((1,), dtype=torch.int32, device=self.device)
            opt = _emst_lib.EmstOptions()
            opt.d_core_dist = _address(core_dist, spare)
            opt.d_u, opt.d_v, opt.d_w = _address(u, spare), _address(v, spare), _address(w, spare)
            opt.d_component = _address(comp, spare)
            opt.max_rounds = int(max_rounds)
            info = _emst_lib.EmstInfo()
            _lib.check(_emst_lib.load().tknnEmst(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        edges = int(info.edges)
        out = {"u": u[:edges], "v": v[:edges], "w": w[:edges], "edges": edges, "info": info.as_dict()}
        if want_components:
            out["components"] = comp
        return out

    def _records(self, who, u, v, w, n, need_w):
        """The records (u, v, w) of ``who`` as the library takes them: contiguous int32 / int32 / float32 tensors of one length on
        the engine's device (numpy is uploaded); at most n - 1 of them."""
        torch = self._torch
        out = []
        for name, t, dtype in (("u", u, torch.int32), ("v", v, torch.int32), ("w", w, torch.float32)):
            if t is None and name == "w" and not need_w:
                out.append(None)
                continue
            if isinstance(t, np.ndarray):
                t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32 if dtype == torch.int32 else np.float32)).to(self.device)
            if not isinstance(t, torch.Tensor):
                raise ValueError("%s: %s must be a numpy array or a torch tensor" % (who, name))
            if t.dtype != dtype or t.dim() != 1 or (out and t.shape != out[0].shape):
                raise ValueError("%s: u, v must be int32 and w float32, all (edges,); got %s %s %s" % (who, name, t.dtype, tuple(t.shape)))
            if t.device != self.device:
                raise ValueError("%s: %s is on %s, the engine on %s" % (who, name, t.device, self.device))
            if not t.is_contiguous():
                raise ValueError("%s: %s must be contiguous" % (who, name))
            out.append(t)
        n = int(n)
        if n < 1 or out[0].shape[0] > n - 1:
            raise ValueError("%s: a forest over n >= 1 vertices has at most n - 1 records" % who)
        return out[0], out[1], out[2], n

    def _linkage_arrays(self, n, edges):
        torch = self._torch
        return {"parent": torch.empty((n + edges,), dtype=torch.int32, device=self.device),
                "left": torch.empty((edges,), dtype=torch.int32, device=self.device),
                "right": torch.empty((edges,), dtype=torch.int32, device=self.device),
                "size": torch.empty((edges,), dtype=torch.int32, device=self.device)}

    def linkage(self, u, v, w=None, n=None, max_rounds=0):
        """The single-linkage dendrogram of a sorted forest (tknnLinkage): the records (u[i], v[i]) over the vertices 0 .. n-1 in
        the order ``emst`` returns them (``n`` defaults to the built set's size; no tree is needed).  The nodes are the leaves and
        n + i for record i.  Returns dict(parent (n + edges,), left, right, size (edges,) int32, info[, w]): parent -1 at roots,
        left < right the children of node n + i, size its leaves; with the weights of a spanning tree ``linkage_matrix`` turns the
        result into scipy's Z.  After ``max_rounds`` contraction rounds (default 64) the rest is finished on the host, with the
        same result (info["host_edges"])."""
        torch = self._torch
        with torch.cuda.device(self.device):
            u, v, w, n = self._records("linkage", u, v, w, self.n if n is None else n, False)
            edges = int(u.shape[0])
            out = self._linkage_arrays(n, edges)
            spare = torch.empty((1,), dtype=torch.int32, device=self.device)
            opt = _hdbscan_lib.LinkageOptions()
            opt.n, opt.edges, opt.max_rounds = n, edges, int(max_rounds)
            opt.d_u, opt.d_v, opt.d_w = _address(u, spare), _address(v, spare), _address(w, spare)
            opt.d_parent = _address(out["parent"], spare)
            opt.d_left, opt.d_right, opt.d_size = _address(out["left"], spare), _address(out["right"], spare), _address(out["size"], spare)
            info = _hdbscan_lib.LinkageInfo()
            _lib.check(_hdbscan_lib.load().tknnLinkage(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        out["info"] = info.as_dict()
        if w is not None:
            out["w"] = w
        return out

    def hdbscan_labels(self, u, v, w, n=None, min_cluster_size=5, max_rounds=0, want_linkage=False, want_lambda=False, want_stability=False):
        """HDBSCAN's labels of a sorted forest (tknnHdbscanLabels): excess-of-mass selection over the condensed tree of the records
        (u, v, w) as ``emst`` returns them (with rows for names), sklearn's ``cluster_selection_method="eom"`` without
        ``allow_single_cluster``; lambda = 1 / w in float64 with w = 0 taken as FLT_MIN, a tie between a cluster and its children
        goes to the cluster.  Returns dict(labels (n,) int32, -1 for noise, clusters numbered by their smallest vertex; info[,
        parent, left, right, size with ``want_linkage``; lam (n,) float64, the lambda at which a point leaves its cluster, with
        ``want_lambda``; stability (edges,) float64, at the node that heads a cluster, with ``want_stability``])."""
        torch = self._torch
        with torch.cuda.device(self.device):
            u, v, w, n = self._records("hdbscan_labels", u, v, w, self.n if n is None else n, True)
            edges = int(u.shape[0])
            out = {"labels": torch.empty((n,), dtype=torch.int32, device=self.device)}
            if want_linkage:
                out.update(self._linkage_arrays(n, edges))
            if want_lambda:
                out["lam"] = torch.empty((n,), dtype=torch.float64, device=self.device)
            if want_stability:
                out["stability"] = torch.empty((edges,), dtype=torch.float64, device=self.device)
            spare = torch.empty((2,), dtype=torch.int32, device=self.device)
            opt = _hdbscan_lib.HdbscanLabelsOptions()
            opt.n, opt.edges, opt.min_cluster_size, opt.max_rounds = n, edges, int(min_cluster_size), int(max_rounds)
            opt.d_u, opt.d_v, opt.d_w = _address(u, spare), _address(v, spare), _address(w, spare)
            opt.d_labels = _address(out["labels"], spare)
            for field, name in (("d_parent", "parent"), ("d_left", "left"), ("d_right", "right"), ("d_size", "size"), ("d_lambda", "lam"),
                                ("d_stability", "stability")):
                setattr(opt, field, _address(out.get(name), spare))
            info = _hdbscan_lib.HdbscanLabelsInfo()
            _lib.check(_hdbscan_lib.load().tknnHdbscanLabels(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        out["info"] = info.as_dict()
        return out

    def hdbscan(self, min_cluster_size=5, min_samples=None, max_rounds=0, want_tree=False, want_linkage=False, want_lambda=False,
                want_core_dist=False, want_stability=False):
        """HDBSCAN of the built set in one call (tknnHdbscan): ``knn`` for the core distances -- the distance to the
        (min_samples - 1)-th nearest other point, sklearn's convention; ``min_samples`` None means ``min_cluster_size``, sklearn's
        default, 1 the plain Euclidean tree --, ``emst`` under them, ``hdbscan_labels`` of its records.  A point that is in no
        record (a NaN coordinate, fewer than min_samples - 1 other points in reach) is noise and counted in info["excluded"].
        Returns dict(labels (n,) int32 by row, info[, u, v, w: ``emst``'s records, by name, with ``want_tree``; parent, left,
        right, size with ``want_linkage`` (leaves are rows); lam with ``want_lambda``; core_dist with ``want_core_dist`` and
        min_samples > 1; stability with ``want_stability``])."""
        torch = self._torch
        n = self.n
        min_cluster_size = int(min_cluster_size)
        min_samples = min_cluster_size if min_samples is None else int(min_samples)
        rows = max(n - 1, 0)
        with torch.cuda.device(self.device):
            out = {"labels": torch.empty((n,), dtype=torch.int32, device=self.device)}
            if want_tree:
                out["u"] = torch.empty((rows,), dtype=torch.int32, device=self.device)
                out["v"] = torch.empty((rows,), dtype=torch.int32, device=self.device)
                out["w"] = torch.empty((rows,), dtype=torch.float32, device=self.device)
            if want_linkage:
                out.update(self._linkage_arrays(n, rows))
            if want_lambda:
                out["lam"] = torch.empty((n,), dtype=torch.float64, device=self.device)
            if want_core_dist and min_samples > 1:
                out["core_dist"] = torch.empty((n,), dtype=torch.float32, device=self.device)
            if want_stability:
                out["stability"] = torch.empty((rows,), dtype=torch.float64, device=self.device)
            spare = torch.empty((2,), dtype=torch.int32, device=self.device)
            opt = _hdbscan_lib.HdbscanOptions()
            opt.min_cluster_size, opt.min_samples, opt.max_rounds = min_cluster_size, min_samples, int(max_rounds)
            for field, name in (("d_labels", "labels"), ("d_core_dist", "core_dist"), ("d_u", "u"), ("d_v", "v"), ("d_w", "w"), ("d_parent", "parent"),
                                ("d_left", "left"), ("d_right", "right"), ("d_size", "size"), ("d_lambda", "lam"), ("d_stability", "stability")):
                setattr(opt, field, _address(out.get(name), spare))
            info = _hdbscan_lib.HdbscanInfo()
            _lib.check(_hdbscan_lib.load().tknnHdbscan(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        edges = int(info.edges)
        for name in ("u", "v", "w", "left", "right", "size", "stability"):
            if name in out:
                out[name] = out[name][:edges]
        if "parent" in out:
            out["parent"] = out["parent"][:n + edges]
        out["edges"] = edges
        out["info"] = info.as_dict()
        return out

    def periodic_knn(self, queries=None, k=1, lo=(0, 0, 0), period=None, radius=None, radii=None, skip_ids=None, want_dist=True):
        """At most ``k`` nearest points of the built set in a periodic cell, as dense rows (tknnPeriodicKnn): ``knn`` and
        ``radius_knn`` under the wrapped distance.  The cell is ``lo`` and ``period`` (three values each; 2-D data: two, z stays
        open); axis a is periodic iff period[a] > 0, 0 means open -- scipy's ``cKDTree(data, boxsize=L)`` is ``lo=0, period=L``.
        Per axis a = |p - q| and w = min(a, |period - a|) on a periodic axis, the distance is sqrt((wx*wx + wy*wy) + wz*wz) in
        fp32; row j holds the points with a finite distance <= r_j, ascending in (distance, index), cut after k and padded with
        idx -1 / dist +inf.  The built set must lie in the cell on every periodic axis (nothing is wrapped for the caller); a
        query outside the cell, or one with a NaN, has an empty row.  At most one of ``radius`` (one for all rows) and ``radii``
        (length m; a row whose radius is NaN, not finite or <= 0 is empty) is given; neither: no radius, the exact k nearest.
        ``queries``, ``skip_ids``: as ``knn`` takes them; without ``queries`` row j answers for point j of the built set, every
        point left out of its own row.  Returns dict(idx (m,k) int32, dist (m,k) float32 [with ``want_dist``], counts (m,) int32,
        info)."""
        torch = self._torch
        if period is None:
            raise ValueError("periodic_knn: give the cell's periods (0 for an open axis)")
        if radius is not None and radii is not None:
            raise ValueError("periodic_knn: give at most one of radius and radii")
        def triple(values, name):
            v = np.atleast_1d(np.asarray(values, np.float64))
            v = np.repeat(v, 3) if v.shape == (1,) else v
            if v.shape not in ((2,), (3,)):
                raise ValueError("periodic_knn: %s must have two or three values (or be one for all axes)" % name)
            return [float(x) for x in v] + [0.0] * (3 - len(v))

        cell = [triple(lo, "lo"), triple(period, "period")]
        if queries is None:
            if skip_ids is not None:
                raise ValueError("periodic_knn: skip_ids go with queries (without queries every point is left out of its own row)")
            m = self.n
        else:
            queries = self._queries(queries, "periodic_knn")
            m = int(queries.shape[0])
        k = int(k)

        def column(values, dtype, name):
            if isinstance(values, torch.Tensor) and values.device != self.device:
                raise ValueError("periodic_knn: %s is on %s, the engine on %s" % (name, values.device, self.device))
            values = torch.as_tensor(values, device=self.device).to(dtype).contiguous()
            if values.shape != (m,):
                raise ValueError("periodic_knn: %s must have one entry per query" % name)
            return values

        with torch.cuda.device(self.device):
            radii = None if radii is None else column(radii, torch.float32, "radii")
            skip_ids = None if skip_ids is None else column(skip_ids, torch.int32, "skip_ids")
            rows = max(k, 0)
            out = {"idx": torch.empty((m, rows), dtype=torch.int32, device=self.device)}
            if want_dist:
                out["dist"] = torch.empty((m, rows), dtype=torch.float32, device=self.device)
            out["counts"] = torch.empty((m,), dtype=torch.int32, device=self.device)
            spare = torch.empty((1,), dtype=torch.int32, device=self.device)
            opt = _periodic_lib.PeriodicKnnOptions()
            opt.m, opt.k = m, k
            opt.radius = float(np.finfo(np.float32).max) if radius is None else float(radius)
            opt.lo, opt.period = (ctypes.c_float * 3)(*cell[0]), (ctypes.c_float * 3)(*cell[1])
            opt.d_queries = None if queries is None else _address(queries, spare)
            opt.d_radii = _address(radii, spare)
            opt.d_skip_ids = _address(skip_ids, spare)
            opt.d_idx = _address(out["idx"], spare)
            opt.d_dist = _address(out.get("dist"))
            opt.d_counts = _address(out["counts"])
            info = _periodic_lib.PeriodicKnnInfo()
            _lib.check(_periodic_lib.load().tknnPeriodicKnn(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        out["info"] = info.as_dict()
        return out

    def batch_knn(self, queries=None, k=1, batch=None, radius=None, radii=None, skip_ids=None, want_dist=True):
        """At most ``k`` nearest points of the query's own batch, as dense rows (tknnBatchKnn), on a tree built with
        ``build(points, batch=...)``: ``knn`` and ``radius_knn`` among the points that carry the query's label -- what
        torch-cluster's ``knn(x, y, k, batch_x, batch_y)`` and ``radius(..., batch_x, batch_y, max_num_neighbors)`` answer.
        Row j holds the points p with batch[p] == batch[j] whose fp32 distance sqrt((dx*dx + dy*dy) + dz*dz) is finite and
        <= r_j, ascending in (distance, index), cut after k and padded with idx -1 / dist +inf.  ``queries`` (numpy (m,2|3) or
        a contiguous float32 CUDA tensor (m,3)) come with ``batch`` ((m,) int32 labels); a query with a NaN, with a label no
        batch has, or in an empty batch has an empty row.  At most one of ``radius`` (one for all rows) and ``radii`` (length
        m; a row whose radius is NaN, not finite or <= 0 is empty) is given; neither: no radius, the exact k nearest of the
        batch.  ``skip_ids``: as ``knn`` takes them.  Without ``queries`` (and ``batch``) row j answers for point j of the built
        set in its own batch, every point left out of its own row.  Returns dict(idx (m,k) int32, dist (m,k) float32 [with
        ``want_dist``], counts (m,) int32, info)."""
        torch = self._torch
        if radius is not None and radii is not None:
            raise ValueError("batch_knn: give at most one of radius and radii")
        if (queries is None) != (batch is None):
            raise ValueError("batch_knn: queries and batch go together (neither: the set's own points)")
        if queries is None:
            if skip_ids is not None:
                raise ValueError("batch_knn: skip_ids go with queries (without queries every point is left out of its own row)")
            m = self.n
        else:
            queries = self._queries(queries, "batch_knn")
            m = int(queries.shape[0])
        k = int(k)

        def column(values, dtype, name):
            if isinstance(values, torch.Tensor) and values.device != self.device:
                raise ValueError("batch_knn: %s is on %s, the engine on %s" % (name, values.device, self.device))
            values = torch.as_tensor(values, device=self.device).to(dtype).contiguous()
            if values.shape != (m,):
                raise ValueError("batch_knn: %s must have one entry per query" % name)
            return values

        with torch.cuda.device(self.device):
            batch = None if batch is None else self._labels(batch, m, "batch_knn", "batch", "query")
            radii = None if radii is None else column(radii, torch.float32, "radii")
            skip_ids = None if skip_ids is None else column(skip_ids, torch.int32, "skip_ids")
            rows = max(k, 0)
            out = {"idx": torch.empty((m, rows), dtype=torch.int32, device=self.device)}
            if want_dist:
                out["dist"] = torch.empty((m, rows), dtype=torch.float32, device=self.device)
            out["counts"] = torch.empty((m,), dtype=torch.int32, device=self.device)
            spare = torch.empty((1,), dtype=torch.int32, device=self.device)
            opt = _batch_lib.BatchKnnOptions()
            opt.m, opt.k = m, k
            opt.radius = float(np.finfo(np.float32).max) if radius is None else float(radius)
            opt.d_queries = None if queries is None else _address(queries, spare)
            opt.d_query_batch = _address(batch, spare)
            opt.d_radii = _address(radii, spare)
            opt.d_skip_ids = _address(skip_ids, spare)
            opt.d_idx = _address(out["idx"], spare)
            opt.d_dist = _address(out.get("dist"))
            opt.d_counts = _address(out["counts"])
            info = _batch_lib.BatchKnnInfo()
            _lib.check(_batch_lib.load().tknnBatchKnn(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        out["info"] = info.as_dict()
        return out

    def fps(self, num_samples=None, ratio=None, num=None, start_rows=None, want_dist=True, prune=True):
        """Farthest point sampling inside each cloud of the built tree (tknnFps; torch-cluster's ``fps(x, batch, ratio)``): the
        B batches of a tree built with ``build(points, batch=...)``, one cloud otherwise.  Row b starts with the cloud's point
        of the smallest name (id, or row without ids) -- or with row ``start_rows[b]`` of the built buffer where that is a
        point of cloud b without a NaN; negative: the default -- and goes on with the unchosen point farthest from those
        chosen, fp32 squared distance (dx*dx + dy*dy) + dz*dz, equal distances decided by the smaller name.  ``num_samples``
        (S): at most that many per cloud; ``num`` ((B,) int32): the samples wanted of each cloud, clipped to 0 .. min(S, n_b);
        ``ratio`` instead of both: ceil(ratio * n_b) of every cloud, computed on the host in float64 from ``batch_layout()``'s
        starts.  ``prune=False`` visits every block of a cloud for every sample (the A/B switch; same results).  Returns
        dict(idx (B,S) int32 padded with -1, dist (B,S) float32 [with ``want_dist``]: the distance to the nearest earlier
        sample, +inf first and in the padding, counts (B,) int32, info)."""
        torch = self._torch
        B = self.num_clouds
        if ratio is not None:
            if num_samples is not None or num is not None:
                raise ValueError("fps: give ratio, or num_samples and/or num")
            if B > 1 or self._is_batched():
                starts = self.batch_layout()["starts"].cpu().numpy().astype(np.int64)
                sizes = starts[1:] - starts[:-1]
            else:
                sizes = np.array([self.n - self._nan_count()], np.int64)
            num = np.ceil(np.float64(ratio) * sizes.astype(np.float64)).astype(np.int64).clip(0, sizes).astype(np.int32)
            num_samples = max(int(num.max()) if len(num) else 1, 1)
        elif num_samples is None:
            if num is None:
                raise ValueError("fps: give num_samples, ratio or num")
            num_samples = max(int(torch.as_tensor(num).max()), 1)

        def column(values, name):
            if isinstance(values, torch.Tensor) and values.device != self.device:
                raise ValueError("fps: %s is on %s, the engine on %s" % (name, values.device, self.device))
            values = torch.as_tensor(values, device=self.device).to(torch.int32).contiguous()
            if values.shape != (B,):
                raise ValueError("fps: %s must have one entry per cloud" % name)
            return values

        S = int(num_samples)
        with torch.cuda.device(self.device):
            num = None if num is None else column(num, "num")
            start_rows = None if start_rows is None else column(start_rows, "start_rows")
            rows = max(S, 0)
            out = {"idx": torch.empty((B, rows), dtype=torch.int32, device=self.device)}
            if want_dist:
                out["dist"] = torch.empty((B, rows), dtype=torch.float32, device=self.device)
            out["counts"] = torch.empty((B,), dtype=torch.int32, device=self.device)
            spare = torch.empty((1,), dtype=torch.int32, device=self.device)
            opt = _fps_lib.FpsOptions()
            opt.num_samples = S
            opt.flags = 0 if prune else _fps_lib.FPS_NO_PRUNE
            opt.d_num = _address(num)
            opt.d_start_rows = _address(start_rows)
            opt.d_idx = _address(out["idx"], spare)
            opt.d_dist = _address(out.get("dist"), spare)
            opt.d_counts = _address(out["counts"])
            info = _fps_lib.FpsInfo()
            _lib.check(_fps_lib.load().tknnFps(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        out["info"] = info.as_dict()
        return out

    def radius_nms(self, radius, scores=None, by_name=False, want_cover=True, max_rounds=0):
        """Greedy suppression within ``radius`` inside each cloud of the built tree (tknnRadiusNms): the kept points are those
        that no stronger kept point of their own cloud has within ``radius`` (fp32 sqrt((dx*dx + dy*dy) + dz*dz) <= radius) --
        non-maximum suppression, a maximal Poisson-disk subset, radius thinning.  A point's strength is ``scores[row]``
        ((n,) float32, numpy or a tensor on the engine's device; a NaN score takes the point out), without scores a hash of
        its name (id, or row without ids), with ``by_name`` nothing: the smallest name wins, which is also what decides among
        equal strengths.  Returns dict(keep (n,) bool by row, idx: the kept names ascending by row (int64, from nonzero on the
        device), cover (n,) int32 [with ``want_cover``]: the name of the nearest kept point within ``radius`` of the point's
        cloud, its own for a kept point, -1 for a point with a NaN, counts (B,) int32: the kept points per cloud, info)."""
        torch = self._torch
        n, B = self.n, self.num_clouds
        with torch.cuda.device(self.device):
            if scores is not None:
                if isinstance(scores, torch.Tensor) and scores.device != self.device:
                    raise ValueError("radius_nms: scores are on %s, the engine on %s" % (scores.device, self.device))
                scores = torch.as_tensor(scores, device=self.device).to(torch.float32).contiguous()
                if tuple(scores.shape) != (n,):
                    raise ValueError("radius_nms: scores must have one entry per built point")
            keep = torch.empty((n,), dtype=torch.uint8, device=self.device)
            out = {"cover": torch.empty((n,), dtype=torch.int32, device=self.device)} if want_cover else {}
            out["counts"] = torch.empty((B,), dtype=torch.int32, device=self.device)
            spare = torch.empty((1,), dtype=torch.int32, device=self.device)
            opt = _nms_lib.RadiusNmsOptions()
            opt.radius = float(radius)
            opt.flags = _nms_lib.NMS_BY_NAME if by_name else 0
            opt.max_rounds = int(max_rounds)
            opt.d_scores = _address(scores, spare)
            opt.d_keep = _address(keep, spare)
            opt.d_cover = _address(out.get("cover"), spare)
            opt.d_counts = _address(out["counts"])
            info = _nms_lib.RadiusNmsInfo()
            _lib.check(_nms_lib.load().tknnRadiusNms(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
            out["keep"] = keep.to(torch.bool)
            rows = torch.nonzero(out["keep"]).reshape(-1)
            out["idx"] = rows if self._row_names is None else self._row_names[rows].to(torch.int64)
        out["info"] = info.as_dict()
        return out

    def radius_reduce(self, radius, queries=None, values=None, weight="one", bandwidth=None, normalize=False, skip_self=False, want_wsum=True,
                      want_counts=True):
        """Sums over the points of the built set within ``radius`` of each query, without the lists (tknnRadiusReduce): the
        neighbours are ``radius_query``'s (fp32 sqrt((dx*dx + dy*dy) + dz*dz) <= radius; nothing is "self").  ``queries``: numpy
        (m,2|3) or a contiguous float32 tensor (m,3) on the engine's device; None: the set's own points, results by row, and
        ``skip_self`` leaves each point out of its own sums.  ``weight``: "one", "gauss" (exp(-d^2 / (2 bandwidth^2)), truncated at
        the radius), "epanechnikov" (1 - d^2 / r^2) or "cubic_spline" (the SPH M4 spline on support r), all unnormalised.
        ``values``: (n,) or (n, C <= 16) float32 by the caller's row -- also on trees built with ids --, numpy or a tensor on the
        engine's device.  ``normalize``: out is divided by the weight sum (0 where that is 0): a kernel-weighted mean.
        Returns dict(out (m, C) float32 -- (m,) for (n,) values, None without values --, wsum (m,) float32 [``want_wsum``],
        counts (m,) int32 [``want_counts``], info)."""
        torch = self._torch
        if weight not in _reduce_lib.WEIGHTS:
            raise ValueError("radius_reduce: weight must be one of %s" % ", ".join(sorted(_reduce_lib.WEIGHTS)))
        if weight == "gauss" and bandwidth is None:
            raise ValueError("radius_reduce: the gauss weight needs a bandwidth")
        if queries is not None:
            queries = self._queries(queries, "radius_reduce")
        m = self.n if queries is None else int(queries.shape[0])
        with torch.cuda.device(self.device):
            flat, C = False, 0
            if values is not None:
                if isinstance(values, torch.Tensor) and values.device != self.device:
                    raise ValueError("radius_reduce: values are on %s, the engine on %s" % (values.device, self.device))
                values = torch.as_tensor(values, device=self.device).to(torch.float32).contiguous()
                flat = values.dim() == 1
                if flat:
                    values = values.reshape(-1, 1)
                if values.dim() != 2 or values.shape[0] != self.n or not 1 <= values.shape[1] <= _reduce_lib.MAX_CHANNELS:
                    raise ValueError("radius_reduce: values must be (n,) or (n, C) with 1 <= C <= %d, one row per built point" % _reduce_lib.MAX_CHANNELS)
                C = int(values.shape[1])
            out = torch.empty((m, C), dtype=torch.float32, device=self.device) if C else None
            wsum = torch.empty((m,), dtype=torch.float32, device=self.device) if want_wsum else None
            counts = torch.empty((m,), dtype=torch.int32, device=self.device) if want_counts else None
            spare = torch.empty((4,), dtype=torch.int32, device=self.device)
            opt = _reduce_lib.RadiusReduceOptions()
            opt.m, opt.radius, opt.bandwidth = m, float(radius), 0.0 if bandwidth is None else float(bandwidth)
            opt.weight, opt.channels = _reduce_lib.WEIGHTS[weight], C
            opt.flags = (_reduce_lib.REDUCE_NORMALIZE if normalize else 0) | (_reduce_lib.REDUCE_SKIP_SELF if skip_self else 0)
            opt.d_queries = None if queries is None else _address(queries, spare)
            opt.d_values = _address(values, spare)
            opt.d_counts, opt.d_wsum, opt.d_out = _address(counts, spare), _address(wsum, spare), _address(out, spare)
            info = _reduce_lib.RadiusReduceInfo()
            _lib.check(_reduce_lib.load().tknnRadiusReduce(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        res = {"out": out.reshape(-1) if (flat and out is not None) else out, "info": info.as_dict()}
        if want_wsum:
            res["wsum"] = wsum
        if want_counts:
            res["counts"] = counts
        return res

    def local_pca(self, radius=None, k=None, queries=None, skip_self=False, viewpoint=None, min_points=3,
                  want=("counts", "centroid", "cov", "eigenvalues", "eigenvectors", "normals", "curvature")):
        """The plane fitted to each query's neighbourhood among the built points, without the lists (tknnLocalPca): the
        neighbourhood is ``radius_query``'s row at ``radius``, ``knn``'s row at ``k``, or with both the entries of the kNN row within
        the radius.  ``queries``: numpy (m,2|3) or a contiguous float32 tensor (m,3) on the engine's device; None: the set's own
        points, results by row -- the point itself is then in its neighbourhood (``k`` counts it: the k nearest including itself)
        unless ``skip_self``.  The moments are sums of the offsets p - q in fp32: counts (m,) int32, centroid (m,3), cov (m,6: xx, xy,
        xz, yy, yz, zz; the population covariance), eigenvalues (m,3) ascending, eigenvectors (m,3,3), row i belonging to
        eigenvalue i, normals (m,3) -- the eigenvector of the smallest eigenvalue, turned towards ``viewpoint`` (three floats) where
        one is given, else so that its largest component is positive --, curvature (m,) = l0 / (l0 + l1 + l2).  Rows with fewer than
        ``min_points`` neighbours have zero eigenvalues, eigenvectors, normal and curvature.
        Returns dict(the outputs named in ``want``, info)."""
        torch = self._torch
        want = tuple(want)
        for name in want:
            if name not in _pca_lib.OUTPUTS:
                raise ValueError("local_pca: want names %r; the outputs are %s" % (name, ", ".join(_pca_lib.OUTPUTS)))
        if viewpoint is not None and len(tuple(viewpoint)) != 3:
            raise ValueError("local_pca: viewpoint must be three floats")
        if queries is not None:
            queries = self._queries(queries, "local_pca")
        m = self.n if queries is None else int(queries.shape[0])
        with torch.cuda.device(self.device):
            spare = torch.empty((4,), dtype=torch.int32, device=self.device)
            opt = _pca_lib.LocalPcaOptions()
            opt.m, opt.radius, opt.k, opt.min_points = m, 0.0 if radius is None else float(radius), 0 if k is None else int(k), int(min_points)
            opt.flags = (_pca_lib.PCA_SKIP_SELF if skip_self else 0) | (_pca_lib.PCA_ORIENT if viewpoint is not None else 0)
            if viewpoint is not None:
                opt.viewpoint[0], opt.viewpoint[1], opt.viewpoint[2] = (float(v) for v in viewpoint)
            opt.d_queries = None if queries is None else _address(queries, spare)
            out = {}
            for name in want:
                field, width = _pca_lib.OUTPUTS[name]
                shape = (m,) if width == 1 else (m, 3, 3) if width == 9 else (m, width)
                out[name] = torch.empty(shape, dtype=torch.int32 if name == "counts" else torch.float32, device=self.device)
                setattr(opt, field, _address(out[name], spare))
            info = _pca_lib.LocalPcaInfo()
            _lib.check(_pca_lib.load().tknnLocalPca(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        out["info"] = info.as_dict()
        return out

    def normals(self, radius=None, k=None, queries=None, skip_self=False, viewpoint=None, min_points=3):
        """``local_pca`` asking for normals, curvature and counts only: dict(normals (m,3), curvature (m,), counts (m,), info)."""
        return self.local_pca(radius=radius, k=k, queries=queries, skip_self=skip_self, viewpoint=viewpoint, min_points=min_points,
                              want=("normals", "curvature", "counts"))

    def fpfh(self, radius, normals=None, normal_radius=None, normal_k=None, self_term=True, want_spfh=False, want_counts=False):
        """The 33-bin Fast Point Feature Histogram of every built point, without the lists (tknnFpfh): three histograms of 11 bins
        over the angles between a point's normal and those of its neighbours within ``radius`` (``radius_query``'s row less the point
        itself), blended with the neighbours' histograms by 1 / d^2 -- Open3D's ``compute_fpfh_feature``; with ``self_term`` False
        PCL's ``FPFHEstimation``.  ``normals``: (n,3) float32 by the caller's row, numpy or a tensor on the engine's device, read as
        given and not normalised; None: exactly one of ``normal_radius`` and ``normal_k`` is given and ``self.normals(...)``
        supplies them.  Returns dict(fpfh (n,33) float32, spfh (n,33) float32 and spfh_counts (n,33) int32 [``want_spfh``],
        counts (n,) int32 [``want_counts``], info)."""
        torch = self._torch
        if normals is None:
            if (normal_radius is None) == (normal_k is None):
                raise ValueError("fpfh: give normals, or exactly one of normal_radius and normal_k")
            normals = self.normals(radius=normal_radius, k=normal_k)["normals"]
        elif normal_radius is not None or normal_k is not None:
            raise ValueError("fpfh: normal_radius and normal_k go without normals")
        n = self.n
        with torch.cuda.device(self.device):
            if isinstance(normals, torch.Tensor) and normals.device != self.device:
                raise ValueError("fpfh: normals are on %s, the engine on %s" % (normals.device, self.device))
            normals = torch.as_tensor(normals, device=self.device).to(torch.float32).contiguous()
            if normals.dim() != 2 or tuple(normals.shape) != (n, 3):
                raise ValueError("fpfh: normals must be (n,3), one row per built point")
            out = {"fpfh": torch.empty((n, _fpfh_lib.FPFH_BINS), dtype=torch.float32, device=self.device)}
            if want_spfh:
                out["spfh"] = torch.empty((n, _fpfh_lib.FPFH_BINS), dtype=torch.float32, device=self.device)
                out["spfh_counts"] = torch.empty((n, _fpfh_lib.FPFH_BINS), dtype=torch.int32, device=self.device)
            if want_counts:
                out["counts"] = torch.empty((n,), dtype=torch.int32, device=self.device)
            spare = torch.empty((4,), dtype=torch.int32, device=self.device)
            opt = _fpfh_lib.FpfhOptions()
            opt.radius, opt.flags = float(radius), 0 if self_term else _fpfh_lib.FPFH_NO_SELF_TERM
            opt.d_normals = _address(normals, spare)
            opt.d_fpfh, opt.d_spfh, opt.d_spfh_counts = _address(out["fpfh"], spare), _address(out.get("spfh"), spare), _address(out.get("spfh_counts"), spare)
            opt.d_counts = _address(out.get("counts"), spare)
            info = _fpfh_lib.FpfhInfo()
            _lib.check(_fpfh_lib.load().tknnFpfh(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        out["info"] = info.as_dict()
        return out

    def icp(self, source, max_dist, init=None, method="point_to_point", target_normals=None, max_iterations=30, rel_fitness=1e-6,
            rel_rmse=1e-6, robust=None, robust_scale=None, want_correspondences=False, want_aligned=False):
        """Rigid registration of ``source`` to the built points by iterated closest points, the loop inside the library (tknnIcp):
        each iteration applies the transform to the source in fp32, finds every point's nearest built point within ``max_dist``
        (``radius_knn`` at k = 1), sums the pairs' moments in fp64 and solves one step -- "point_to_point" (Kabsch / Horn) or
        "point_to_plane" (Gauss-Newton on (s' - p) . n, Open3D's angles), with ``robust`` None / "l2", "huber" or "tukey" at
        ``robust_scale``.  ``source``: numpy (m,2|3) or a contiguous float32 tensor (m,3) on the engine's device.  ``init``: a
        4 x 4 transform (anything np.asarray takes), None: the identity.  ``target_normals``: (n,3) float32 by the caller's row,
        numpy or a tensor on the engine's device (``normals(k=16)["normals"]``); point_to_plane needs them.  The loop stops when
        fitness and inlier_rmse both change by less than ``rel_fitness`` / ``rel_rmse``, after ``max_iterations`` steps, or at a
        degenerate system.  The tree must have been built without ids.
        Returns dict(transform (4,4) float64 CPU tensor, fitness, inlier_rmse, correspondences, iterations, searches, converged,
        degenerate, skipped_pairs, the work counters and times; corr (m,) int32 and corr_dist (m,) float32 of the last search
        [``want_correspondences``]; aligned (m,3) float32 [``want_aligned``])."""
        torch = self._torch
        if method not in _icp_lib.METHODS:
            raise ValueError("icp: method must be one of %s" % ", ".join(sorted(_icp_lib.METHODS)))
        if robust not in _icp_lib.ROBUST:
            raise ValueError("icp: robust must be None, 'l2', 'huber' or 'tukey'")
        if _icp_lib.ROBUST[robust] and robust_scale is None:
            raise ValueError("icp: robust=%r needs a robust_scale" % robust)
        if method == "point_to_plane" and target_normals is None:
            raise ValueError("icp: point_to_plane needs target_normals")
        source = self._queries(source, "icp")
        m = int(source.shape[0])
        t0 = None
        if init is not None:
            t0 = np.ascontiguousarray(init.cpu().numpy() if isinstance(init, torch.Tensor) else init, dtype=np.float64)
            if t0.shape != (4, 4):
                raise ValueError("icp: init must be a 4 x 4 transform, got %s" % (t0.shape,))
        with torch.cuda.device(self.device):
            if target_normals is not None:
                if isinstance(target_normals, np.ndarray):
                    target_normals = torch.from_numpy(np.ascontiguousarray(target_normals, dtype=np.float32)).to(self.device)
                self._written_in_place("icp", "target_normals", target_normals, (self.n, 3), torch.float32)
            spare = torch.empty((4,), dtype=torch.int32, device=self.device)
            corr = torch.empty((m,), dtype=torch.int32, device=self.device) if want_correspondences else None
            corr_dist = torch.empty((m,), dtype=torch.float32, device=self.device) if want_correspondences else None
            aligned = torch.empty((m, 3), dtype=torch.float32, device=self.device) if want_aligned else None
            opt = _icp_lib.IcpOptions()
            opt.m, opt.d_source, opt.d_target_normals = m, _address(source, spare), _address(target_normals, spare)
            opt.init = None if t0 is None else t0.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
            opt.max_dist, opt.robust_scale = float(max_dist), 0.0 if robust_scale is None else float(robust_scale)
            opt.method, opt.robust, opt.max_iterations = _icp_lib.METHODS[method], _icp_lib.ROBUST[robust], int(max_iterations)
            opt.rel_fitness, opt.rel_rmse = float(rel_fitness), float(rel_rmse)
            opt.d_corr, opt.d_corr_dist, opt.d_aligned = _address(corr, spare), _address(corr_dist, spare), _address(aligned, spare)
            info = _icp_lib.IcpInfo()
            _lib.check(_icp_lib.load().tknnIcp(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        res = info.as_dict()
        res["transform"] = torch.tensor(list(info.transform), dtype=torch.float64).reshape(4, 4)
        if want_correspondences:
            res["corr"], res["corr_dist"] = corr, corr_dist
        if want_aligned:
            res["aligned"] = aligned
        return res

    def evaluate_registration(self, source, max_dist, init=None):
        """``icp`` with no step taken: fitness, inlier_rmse and correspondences of ``source`` under ``init`` (None: as it is)."""
        return self.icp(source, max_dist, init=init, max_iterations=0)

    def _features(self, feat, who, name):
        """The descriptor rows ``name`` of ``who`` as the library takes them: a contiguous float32 (rows, D) tensor on the engine's
        device; numpy is uploaded."""
        torch = self._torch
        if isinstance(feat, np.ndarray):
            feat = torch.from_numpy(np.ascontiguousarray(feat, dtype=np.float32)).to(self.device)
        if not isinstance(feat, torch.Tensor) or feat.dtype != torch.float32 or feat.dim() != 2:
            raise ValueError("%s: %s must be float32 (rows, D), numpy or a tensor" % (who, name))
        if feat.device != self.device:
            raise ValueError("%s: %s is on %s, the engine on %s" % (who, name, feat.device, self.device))
        return feat.contiguous()

    def _match(self, a, b):
        """tknnFeatureMatch of the rows ``a`` against the rows ``b``: (best, best_d2, second_d2, info)."""
        torch = self._torch
        m, n, D = int(a.shape[0]), int(b.shape[0]), int(a.shape[1])
        best = torch.empty((m,), dtype=torch.int32, device=self.device)
        best_d2 = torch.empty((m,), dtype=torch.float32, device=self.device)
        second_d2 = torch.empty((m,), dtype=torch.float32, device=self.device)
        spare = torch.empty((4,), dtype=torch.int32, device=self.device)
        opt = _global_lib.FeatureMatchOptions()
        opt.m, opt.n, opt.D = m, n, D
        opt.d_source, opt.d_target = _address(a, spare), _address(b, spare)
        opt.d_best, opt.d_best_d2, opt.d_second_d2 = _address(best, spare), _address(best_d2, spare), _address(second_d2, spare)
        info = _global_lib.FeatureMatchInfo()
        _lib.check(_global_lib.load().tknnFeatureMatch(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        return best, best_d2, second_d2, info.as_dict()

    def match_features(self, source_feat, target_feat, mutual=False, ratio=None, want_dist=False):
        """The nearest and second-nearest row of ``target_feat`` (n, D) for every row of ``source_feat`` (m, D), D <= 64, by brute
        force in literal fp32 (tknnFeatureMatch; no tree is needed): the matching step between ``fpfh`` and ``ransac``.  Rows are
        numpy or float32 tensors on the engine's device; a row with an entry that is not finite matches nobody.
        ``mutual``: a second call with the roles swapped, and only the rows i with best_t[best_s[i]] == i are kept.
        ``ratio``: only the rows with best_d2 <= ratio^2 * second_d2 are kept (Lowe's test on the distances).
        Returns dict(pairs (c,2) int32 on the device: source row, target row of the rows kept, in row order; best (m,) int32,
        -1 for no match; best_d2, second_d2 (m,) float32 squared distances; info[, dist (c,) float32: the distance of each pair,
        ``want_dist``])."""
        torch = self._torch
        with torch.cuda.device(self.device):
            a, b = self._features(source_feat, "match_features", "source_feat"), self._features(target_feat, "match_features", "target_feat")
            if a.shape[1] != b.shape[1]:
                raise ValueError("match_features: source_feat has %d channels, target_feat %d" % (a.shape[1], b.shape[1]))
            best, best_d2, second_d2, info = self._match(a, b)
            keep = best >= 0
            if mutual:
                back, _, _, info_back = self._match(b, a)
                rows = torch.arange(a.shape[0], dtype=torch.int32, device=self.device)
                if b.shape[0] > 0:  # (no target rows: nobody has a best, and there is nothing to index)
                    keep &= back[best.clamp(min=0).long()] == rows
                info["swapped"] = info_back
            if ratio is not None:
                keep &= best_d2 <= float(np.float32(float(ratio) ** 2)) * second_d2  # (ratio^2 rounded to fp32, the product fp32)
            rows = torch.nonzero(keep).reshape(-1)
            out = {"pairs": torch.stack([rows.to(torch.int32), best[rows]], dim=1).contiguous(), "best": best, "best_d2": best_d2, "second_d2": second_d2,
                   "info": info}
            if want_dist:
                out["dist"] = torch.sqrt(best_d2[rows])
        return out

    def ransac(self, source, target, pairs, max_dist, ransac_n=3, edge_similarity=0.9, max_trials=100000, confidence=0.999, seed=0, refit_rounds=2,
               want_mask=False, want_trials=False):
        """RANSAC over correspondences on the device (tknnRansac; no tree is needed): the rigid transform that maps ``source`` rows
        onto the ``target`` rows ``pairs`` (c,2) int32 names them with, up to ``max_dist``, for the most pairs.  Trials run in
        batches of 4096: a sample of ``ransac_n`` (3 or 4) pairs drawn by a counter-based hash of ``seed`` and the trial, rejected
        early unless its edge lengths agree within ``edge_similarity`` (0: no check), solved by Kabsch / Horn in double, and scored
        against every pair; the loop stops once ``confidence`` is reached or after ``max_trials``; the best is refitted to its
        inliers up to ``refit_rounds`` times.  ``source``, ``target``: numpy (rows,2|3) or contiguous float32 tensors (rows,3) on the
        engine's device.  Returns dict(transform (4,4) float64 CPU tensor -- ``icp``'s ``init`` --, best_trial (-1: no sample
        survived, transform is the identity), inliers, fitness, inlier_rmse, trials_run, batches, status_counts by
        _global_lib.STATUS, refits_kept, the times; mask (c,) uint8 under the final transform [``want_mask``]; trial_status and
        trial_inliers (max_trials,) int32, -1 where not run or not scored [``want_trials``])."""
        torch = self._torch
        source, target = self._queries(source, "ransac"), self._queries(target, "ransac")
        with torch.cuda.device(self.device):
            if isinstance(pairs, np.ndarray):
                pairs = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).to(self.device)
            if not isinstance(pairs, torch.Tensor) or pairs.dim() != 2 or pairs.shape[1] != 2:
                raise ValueError("ransac: pairs must be (c,2): source row, target row")
            self._written_in_place("ransac", "pairs", pairs, tuple(pairs.shape), torch.int32)
            c, trials = int(pairs.shape[0]), int(max_trials)
            spare = torch.empty((4,), dtype=torch.int32, device=self.device)
            mask = torch.empty((c,), dtype=torch.uint8, device=self.device) if want_mask else None
            status = torch.empty((max(trials, 0),), dtype=torch.int32, device=self.device) if want_trials else None
            inliers = torch.empty((max(trials, 0),), dtype=torch.int32, device=self.device) if want_trials else None
            opt = _global_lib.RansacOptions()
            opt.ms, opt.mt, opt.c = int(source.shape[0]), int(target.shape[0]), c
            opt.d_source, opt.d_target, opt.d_pairs = _address(source, spare), _address(target, spare), _address(pairs, spare)
            opt.ransac_n, opt.max_dist, opt.edge_similarity = int(ransac_n), float(max_dist), float(edge_similarity)
            opt.max_trials, opt.confidence, opt.seed, opt.refit_rounds = trials, float(confidence), int(seed) & 0xFFFFFFFF, int(refit_rounds)
            opt.d_inlier_mask, opt.d_trial_status, opt.d_trial_inliers = _address(mask, spare), _address(status, spare), _address(inliers, spare)
            info = _global_lib.RansacInfo()
            _lib.check(_global_lib.load().tknnRansac(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        res = info.as_dict()
        res["transform"] = torch.tensor(list(info.transform), dtype=torch.float64).reshape(4, 4)
        res["status_counts"] = dict(zip(_global_lib.STATUS, info.status_counts))
        if want_mask:
            res["mask"] = mask
        if want_trials:
            res["trial_status"], res["trial_inliers"] = status, inliers
        return res

    def voxel_down_sample(self, points, voxel_size, batch=None, values=None, origin=None, reduce="mean", want_map=False, want_cells=False,
                          max_voxels=None, num_batches=None):
        """One point per occupied cell of a grid of edge ``voxel_size``, inside each cloud (tknnVoxelGrid; no tree is needed, and a
        built one is left alone): Open3D's ``voxel_down_sample``, PCL's ``VoxelGrid``, torch-cluster's ``grid_cluster`` followed by
        ``avg_pool``.  ``points``: numpy (n,2|3) or a contiguous float32 (n,3) tensor on the engine's device.  The cell of a row is
        floorf((p - origin) / voxel_size) per axis in fp32; a row with a coordinate that is not finite, with a label outside
        [0, num_batches) or with a cell outside [0, 2^21) is left out.  ``batch``: (n,) int32 labels in any order, no voxel spans
        two clouds (``num_batches`` defaults to the largest label + 1).  ``values``: (n, C) float32, C <= 16, reduced with the
        points.  ``origin``: the grid's corner; None: the minimum of the finite points minus ``voxel_size / 2`` (Open3D's).
        ``reduce``: "mean" -- the fp64 centroid of the cell's rows and the mean of their values, rounded once; "first" -- the cell's
        smallest row; "nearest" -- its row nearest to the centroid, ties to the smaller row; "center" -- origin + (cell + 0.5) *
        voxel_size, the values averaged.  Voxels are ordered by (label, cx, cy, cz), whatever the order of the rows.
        ``max_voxels``: the capacity of the outputs (more voxels: the call is refused); None: n, and views of the first V rows come
        back -- one call, one sort.
        Returns dict(points (V,3) float32, counts (V,) int32, offsets (num_batches + 1,) int64: the voxels of each cloud, info
        [, values (V,C); rows (V,) int32, the rows kept, for "first" and "nearest"; batch (V,) int32 with ``batch``; map (n,) int32,
        the voxel of each row, -1 for a row left out, ``want_map``; cells (V,3) int32, ``want_cells``]), tensors on the device."""
        torch = self._torch
        if reduce not in ("mean", "first", "nearest", "center"):
            raise ValueError('voxel_down_sample: reduce must be "mean", "first", "nearest" or "center"')
        if not float(voxel_size) > 0 or not np.isfinite(np.float32(voxel_size)):
            raise ValueError("voxel_down_sample: voxel_size must be finite and > 0")
        points = self._queries(points, "voxel_down_sample")
        n = int(points.shape[0])
        with torch.cuda.device(self.device):
            B = 1
            if batch is not None:
                batch = self._labels(batch, n, "voxel_down_sample", "batch", "point")
                B = int(num_batches) if num_batches is not None else (int(batch.max()) + 1 if n > 0 else 1)
                B = max(B, 1)  # (a negative label is left out by the library)
            elif num_batches is not None:
                raise ValueError("voxel_down_sample: num_batches goes with batch")
            C = 0
            if values is not None:
                values = self._features(values, "voxel_down_sample", "values")
                C = int(values.shape[1])
                if values.shape[0] != n or C < 1 or C > _voxel_lib.VOXEL_MAX_CHANNELS:
                    raise ValueError("voxel_down_sample: values must be (n, C) with 1 <= C <= %d" % _voxel_lib.VOXEL_MAX_CHANNELS)
            voxel = torch.tensor(float(voxel_size), dtype=torch.float32, device=self.device)
            if origin is None:
                finite = torch.isfinite(points).all(dim=1, keepdim=True)
                if n > 0 and bool(finite.any()):
                    lo = torch.where(finite, points, torch.full_like(points, float("inf"))).min(dim=0).values
                    origin = (lo - voxel / 2).tolist()
                else:
                    origin = [0.0, 0.0, 0.0]
            origin = [float(np.float32(x)) for x in origin]
            if len(origin) != 3:
                raise ValueError("voxel_down_sample: origin must have three entries")
            cap = n if max_voxels is None else int(max_voxels)
            mean = reduce in ("mean", "center")

            wanted = {"counts": ((cap,), torch.int32), "offsets": ((B + 1,), torch.int64)}
            if reduce == "mean":
                wanted["centroid"] = ((cap, 3), torch.float32)
            if want_cells or reduce == "center":
                wanted["cells"] = ((cap, 3), torch.int32)
            if C > 0 and mean:
                wanted["value_mean"] = ((cap, C), torch.float32)
            if not mean:
                wanted["rows"] = ((cap,), torch.int32)
            if batch is not None:
                wanted["labels"] = ((cap,), torch.int32)
            if want_map:
                wanted["map"] = ((n,), torch.int32)
            bufs = _call_outputs(torch, self.device, wanted)
            counts, centroid, cells, value_mean, rows = (bufs.get(k) for k in ("counts", "centroid", "cells", "value_mean", "rows"))
            labels, offsets, vmap, spare = (bufs.get(k) for k in ("labels", "offsets", "map", "spare"))
            opt = _voxel_lib.VoxelGridOptions()
            opt.n, opt.d_points, opt.d_batch, opt.d_values = n, _address(points, spare), _address(batch, spare), _address(values, spare)
            opt.voxel, opt.num_batches, opt.channels, opt.capacity = float(voxel_size), B, C, cap
            for axis in range(3):
                opt.origin[axis] = origin[axis]
            opt.d_count, opt.d_centroid, opt.d_cell, opt.d_value_mean = _address(counts, spare), _address(centroid, spare), _address(cells, spare), _address(value_mean, spare)
            opt.d_first = _address(rows, spare) if reduce == "first" else None
            opt.d_nearest = _address(rows, spare) if reduce == "nearest" else None
            opt.d_voxel_label, opt.d_offsets, opt.d_map = _address(labels, spare), _address(offsets, spare), _address(vmap, spare)
            info = _voxel_lib.VoxelGridInfo()
            _lib.check(_voxel_lib.load().tknnVoxelGrid(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
            res = info.as_dict()
            V = int(info.voxels)
            if reduce == "mean":
                pts = centroid[:V]
            elif reduce == "center":
                pts = torch.tensor(origin, dtype=torch.float32, device=self.device) + (cells[:V].to(torch.float32) + 0.5) * voxel
            else:
                pts = points[rows[:V].long()]
            result = {"points": pts, "counts": counts[:V], "offsets": offsets, "info": res}
            if C > 0:
                result["values"] = value_mean[:V] if mean else values[rows[:V].long()]
            if not mean:
                result["rows"] = rows[:V]
            if batch is not None:
                result["batch"] = labels[:V]
            if want_map:
                result["map"] = vmap
            if want_cells:
                result["cells"] = cells[:V]
        return result

    def orient_normals(self, normals, k=16, direction=(0, 0, 1), emst=True, want=("normals", "flip"), in_place=False, max_rounds=0):
        """One consistent sign per normal of the built set, with no viewpoint (tknnOrientNormals): Hoppe's propagation, Open3D's
        ``orient_normals_consistent_tangent_plane(k)``.  The graph joins every point to its ``k`` nearest others (``knn``'s own rows)
        and, with ``emst``, by the records of the Euclidean ``emst``, so that it is connected wherever that forest is; an edge weighs
        1 - |n_i . n_j| in fp32, edges are ordered by (bits of the weight, smaller name, larger name), and along the unique minimum
        spanning forest under that order every normal is flipped to agree with its tree parent.  The root of a component is its point
        farthest along ``direction`` (the smallest row among equals), flipped iff its normal points against it.  ``normals``: (n,3)
        float32 by the caller's row, numpy or a tensor on the engine's device, read as given; a point with a NaN coordinate or a normal
        that is not finite takes no part and keeps its normal.  The result does not depend on the signs of the input.
        ``want``: any of "normals", "flip", "components", "tree"; ``in_place`` writes the normals over ``normals`` (a contiguous
        float32 tensor on the engine's device) and returns that tensor.  Returns dict(normals (n,3) float32, flip (n,) uint8,
        components (n,) int32: the smallest row of the point's component of the graph, -1 for a point left out, u, v (tree_edges,)
        int32 with u < v and w (tree_edges,) float32: the forest's records ascending by the key, info)."""
        torch = self._torch
        want = (want,) if isinstance(want, str) else tuple(want)
        unknown = set(want) - {"normals", "flip", "components", "tree"}
        if unknown:
            raise ValueError("orient_normals: want has %s; it takes normals, flip, components, tree" % sorted(unknown))
        if in_place and "normals" not in want:
            raise ValueError('orient_normals: in_place goes with "normals" in want')
        if "normals" not in want and "flip" not in want:
            raise ValueError('orient_normals: want needs "normals" or "flip"')
        direction = [float(np.float32(x)) for x in direction]
        if len(direction) != 3:
            raise ValueError("orient_normals: direction must have three entries")
        n = self.n
        with torch.cuda.device(self.device):
            if in_place:
                self._written_in_place("orient_normals", "normals", normals, (n, 3), torch.float32)
            else:
                if isinstance(normals, torch.Tensor) and normals.device != self.device:
                    raise ValueError("orient_normals: normals are on %s, the engine on %s" % (normals.device, self.device))
                normals = torch.as_tensor(normals, device=self.device).to(torch.float32).contiguous()
                if normals.dim() != 2 or tuple(normals.shape) != (n, 3):
                    raise ValueError("orient_normals: normals must be (n,3), one row per built point")
            rows = max(n - 1, 0)
            wanted = {}
            if "normals" in want and not in_place:
                wanted["normals"] = ((n, 3), torch.float32)
            if "flip" in want:
                wanted["flip"] = ((n,), torch.uint8)
            if "components" in want:
                wanted["components"] = ((n,), torch.int32)
            if "tree" in want:
                wanted.update({"u": ((rows,), torch.int32), "v": ((rows,), torch.int32), "w": ((rows,), torch.float32)})
            out = _call_outputs(torch, self.device, wanted)
            spare = out.pop("spare")
            if in_place:
                out["normals"] = normals
            opt = _orient_lib.OrientOptions()
            opt.d_normals = _address(normals, spare)
            opt.k, opt.flags, opt.max_rounds = int(k), 0 if emst else _orient_lib.ORIENT_NO_EMST, int(max_rounds)
            for axis in range(3):
                opt.direction[axis] = direction[axis]
            opt.d_out_normals, opt.d_flip, opt.d_component = _address(out.get("normals"), spare), _address(out.get("flip"), spare), _address(out.get("components"), spare)
            opt.d_u, opt.d_v, opt.d_w = _address(out.get("u"), spare), _address(out.get("v"), spare), _address(out.get("w"), spare)
            info = _orient_lib.OrientInfo()
            _lib.check(_orient_lib.load().tknnOrientNormals(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        if "tree" in want:
            edges = int(info.tree_edges)
            out["u"], out["v"], out["w"] = out["u"][:edges], out["v"][:edges], out["w"][:edges]
        out["info"] = info.as_dict()
        return out

    def segment_plane(self, distance_threshold, num_iterations=1000, confidence=0.999, seed=0, active=None, axis=None, max_angle=None, refit_rounds=1,
                      want=("plane", "inliers"), return_info=False):
        """The plane most rows of the built set lie within ``distance_threshold`` of, by RANSAC on the device (tknnSegmentPlane): Open3D's
        ``segment_plane(distance_threshold, 3, num_iterations)``, PCL's ``SACSegmentation`` with ``SACMODEL_PLANE`` and, with ``axis``
        and ``max_angle`` (radians between the plane's normal and the axis), ``SACMODEL_PERPENDICULAR_PLANE``.  Trials run in batches
        of 1024: three rows drawn by a counter-based hash of ``seed`` and the trial, the plane through them, its inliers counted by a
        walk of the box pyramid that skips boxes outside the slab and counts boxes inside it by arithmetic; the loop stops once
        ``confidence`` is reached (1: never early) or after ``num_iterations``; the best plane is refitted to its inliers up to
        ``refit_rounds`` times.  ``active``: (n,) uint8 or bool by row, numpy or a tensor on the engine's device -- only rows with a
        nonzero entry (and finite coordinates) are sampled, scored and reported; the tree is never rebuilt.
        Returns (plane, rows): plane a (4,) float64 CPU tensor (a, b, c, d) with a*x + b*y + c*z + d = 0 and a unit normal turned
        towards ``axis`` (without one: its first nonzero entry positive), all zero when no sample gave a plane; rows the (inliers,)
        int32 inlier rows ascending, on the device.  ``return_info``: a dict instead -- plane, rows [``"inliers"`` in ``want``], mask
        (n,) uint8 [``"mask"``], trial_status and trial_inliers (num_iterations,) int32, -1 where not run or not scored
        [``"trials"``], info (best_trial, inliers, active, fitness, inlier_rmse, status_counts by _plane_lib.STATUS, the work
        counters, the times)."""
        torch = self._torch
        want = (want,) if isinstance(want, str) else tuple(want)
        unknown = set(want) - {"plane", "inliers", "mask", "trials"}
        if unknown:
            raise ValueError("segment_plane: want has %s; it takes plane, inliers, mask, trials" % sorted(unknown))
        if (axis is None) != (max_angle is None):
            raise ValueError("segment_plane: axis and max_angle go together")
        n, trials = self.n, int(num_iterations)
        with torch.cuda.device(self.device):
            if active is not None:
                if isinstance(active, torch.Tensor) and active.device != self.device:
                    raise ValueError("segment_plane: active is on %s, the engine on %s" % (active.device, self.device))
                active = torch.as_tensor(active, device=self.device)
                if active.dim() != 1 or active.shape[0] != n or active.dtype not in (torch.uint8, torch.bool):
                    raise ValueError("segment_plane: active must be (n,) uint8 or bool, one entry per built point")
                active = active.to(torch.uint8).contiguous()
            wanted = {}
            if "inliers" in want:
                wanted["rows"] = ((n,), torch.int32)
            if "mask" in want:
                wanted["mask"] = ((n,), torch.uint8)
            if "trials" in want:
                wanted.update({"trial_status": ((max(trials, 0),), torch.int32), "trial_inliers": ((max(trials, 0),), torch.int32)})
            out = _call_outputs(torch, self.device, wanted)
            spare = out.pop("spare")
            opt = _plane_lib.PlaneOptions()
            opt.d_active = _address(active, spare)
            opt.distance_threshold, opt.max_trials, opt.confidence = float(distance_threshold), trials, float(confidence)
            opt.seed, opt.refit_rounds = int(seed) & 0xFFFFFFFF, int(refit_rounds)
            if axis is not None:
                axis = [float(np.float32(x)) for x in axis]
                if len(axis) != 3 or not any(axis):
                    raise ValueError("segment_plane: axis must have three entries, not all zero")
                for i in range(3):
                    opt.axis[i] = axis[i]
                opt.min_cos = float(np.cos(float(max_angle)))
            opt.d_inlier_rows, opt.d_inlier_mask = _address(out.get("rows"), spare), _address(out.get("mask"), spare)
            opt.d_trial_status, opt.d_trial_inliers = _address(out.get("trial_status"), spare), _address(out.get("trial_inliers"), spare)
            info = _plane_lib.PlaneInfo()
            _lib.check(_plane_lib.load().tknnSegmentPlane(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        res = info.as_dict()
        plane = torch.tensor(list(info.plane), dtype=torch.float64)
        res["plane"], res["normal"], res["anchor"] = list(info.plane), list(info.normal), list(info.anchor)
        res["status_counts"] = dict(zip(_plane_lib.STATUS, info.status_counts))
        if "inliers" in want:
            out["rows"] = out["rows"][:int(info.inliers)]
        if not return_info:
            return plane, out.get("rows")
        out["plane"], out["info"] = plane, res
        return out

    def segment_planes(self, distance_threshold, max_planes, min_inliers, active=None, **kw):
        """Up to ``max_planes`` planes of the built set, the largest first: ``segment_plane(distance_threshold, active=..., **kw)``
        again and again, each plane's inliers cleared from an active mask this call owns (a copy of ``active``; None: every row)
        before the next; the tree is never rebuilt.  It stops at the first plane with fewer than ``min_inliers`` inliers, which is
        not reported.  Returns (planes, labels): planes a list of (plane, rows) as ``segment_plane`` returns them, labels (n,) int32
        on the device, the index of the row's plane in that list, -1 for a row in none."""
        torch = self._torch
        if "want" in kw or "return_info" in kw:
            raise ValueError("segment_planes: want and return_info are segment_plane's")
        n = self.n
        with torch.cuda.device(self.device):
            if active is None:
                mask = torch.ones((n,), dtype=torch.uint8, device=self.device)
            else:
                if isinstance(active, torch.Tensor) and active.device != self.device:
                    raise ValueError("segment_planes: active is on %s, the engine on %s" % (active.device, self.device))
                mask = torch.as_tensor(active, device=self.device)
                if mask.dim() != 1 or mask.shape[0] != n or mask.dtype not in (torch.uint8, torch.bool):
                    raise ValueError("segment_planes: active must be (n,) uint8 or bool, one entry per built point")
                mask = (mask != 0).to(torch.uint8)  # (a copy: the caller's stays as it is)
            labels = torch.full((n,), -1, dtype=torch.int32, device=self.device)
            planes = []
            while len(planes) < int(max_planes):
                plane, rows = self.segment_plane(distance_threshold, active=mask, **kw)
                if rows.shape[0] < max(int(min_inliers), 1):
                    break
                labels[rows.long()] = len(planes)
                mask[rows.long()] = 0
                planes.append((plane, rows))
        return planes, labels

    def mean_shift_modes(self, bandwidth, seeds=None, kernel="flat", radius=None, tol=None, max_iterations=300):
        """Mean-shift trajectories over the built set, the loop inside the library (tknnMeanShift): every seed moves to the
        kernel-weighted mean of the built points within ``radius`` of it (fp32 sqrt((dx*dx + dy*dy) + dz*dz) <= radius; the sums
        are over the offsets p - x) until its shift is at most ``tol``, it has no neighbours, or ``max_iterations`` steps are taken.
        ``seeds``: numpy (m,2|3) or a contiguous float32 tensor (m,3) on the engine's device; None: the set's own points, results
        by row.  ``kernel``: "flat" (sklearn's), "gauss" (exp(-d^2 / (2 bandwidth^2)), truncated at the radius) or "epanechnikov"
        (1 - d^2 / r^2).  ``radius`` defaults to ``bandwidth``, for "gauss" to 3 ``bandwidth``; ``tol`` to 1e-3 ``bandwidth``
        (sklearn's).  Returns dict(modes (m,3) float32, counts (m,) int32 and wsum (m,) float32 of the seed's last walk, shift (m,)
        float32 (+inf where no step was taken), iterations (m,) int32, status (m,) uint8 -- 0 still moving at max_iterations, 1
        converged, 2 no neighbours, 3 a NaN --, info)."""
        torch = self._torch
        if kernel not in _meanshift_lib.KERNELS:
            raise ValueError("mean_shift_modes: kernel must be one of %s" % ", ".join(sorted(_meanshift_lib.KERNELS)))
        bandwidth = float(bandwidth)
        if radius is None:
            radius = 3.0 * bandwidth if kernel == "gauss" else bandwidth
        if tol is None:
            tol = 1e-3 * bandwidth
        if seeds is not None:
            seeds = self._queries(seeds, "mean_shift_modes")
        m = self.n if seeds is None else int(seeds.shape[0])
        with torch.cuda.device(self.device):
            out = {"modes": torch.empty((m, 3), dtype=torch.float32, device=self.device),
                   "counts": torch.empty((m,), dtype=torch.int32, device=self.device),
                   "wsum": torch.empty((m,), dtype=torch.float32, device=self.device),
                   "shift": torch.empty((m,), dtype=torch.float32, device=self.device),
                   "iterations": torch.empty((m,), dtype=torch.int32, device=self.device),
                   "status": torch.empty((m,), dtype=torch.uint8, device=self.device)}
            spare = torch.empty((4,), dtype=torch.int32, device=self.device)
            opt = _meanshift_lib.MeanShiftOptions()
            opt.m, opt.radius, opt.bandwidth, opt.tol = m, float(radius), bandwidth, float(tol)
            opt.weight, opt.max_iterations = _meanshift_lib.KERNELS[kernel], int(max_iterations)
            opt.d_seeds = None if seeds is None else _address(seeds, spare)
            for name in _meanshift_lib.OUTPUTS:
                setattr(opt, "d_" + name, _address(out[name], spare))
            info = _meanshift_lib.MeanShiftInfo()
            _lib.check(_meanshift_lib.load().tknnMeanShift(self._h, ctypes.byref(opt), ctypes.byref(info), self._stream()))
        out["info"] = info.as_dict()
        return out

    def mean_shift(self, bandwidth, seeds=None, kernel="flat", radius=None, tol=None, max_iterations=300, merge_radius=None, cluster_all=True,
                   min_count=1, points=None):
        """Mean-shift clustering of the built set, sklearn's ``MeanShift``: ``mean_shift_modes`` for the trajectories, then the
        existing calls for the rest.  The candidates are the seeds that converged with at least ``min_count`` neighbours; among
        candidates within ``merge_radius`` (default: ``bandwidth``) of each other the one with the larger score -- its neighbour
        count, for "gauss" and "epanechnikov" its weight sum -- stays, the smaller row among equal scores (``radius_nms`` on a tree
        of the modes); ``centers`` are the kept modes by descending score, then ascending candidate row.  ``labels``: the nearest
        centre of every point (``knn`` at k = 1 against a tree of the centres); with ``cluster_all`` False only within
        ``bandwidth`` (``radius_knn``), -1 otherwise; a point with a NaN is -1.  ``points``: the built set again, by the caller's
        row (numpy or a tensor on the engine's device) -- the engine keeps no copy by row.  ``seeds`` None: the points themselves.
        Returns dict(centers (c,3) float32, labels (n,) int64, scores (c,) float32, modes, the arrays of ``mean_shift_modes``, info)."""
        torch = self._torch
        if points is None:
            raise ValueError("mean_shift: give points, the built set by the caller's row (the labels are theirs)")
        points = self._points(points)
        if points.shape[0] != self.n:
            raise ValueError("mean_shift: points must be the built set, one row per built point")
        res = self.mean_shift_modes(bandwidth, seeds=seeds, kernel=kernel, radius=radius, tol=tol, max_iterations=max_iterations)
        with torch.cuda.device(self.device):
            cand = torch.nonzero((res["status"] == _meanshift_lib.MS_CONVERGED) & (res["counts"] >= int(min_count))).reshape(-1)
            res["centers"] = torch.empty((0, 3), dtype=torch.float32, device=self.device)
            res["scores"] = torch.empty((0,), dtype=torch.float32, device=self.device)
            res["labels"] = torch.full((self.n,), -1, dtype=torch.int64, device=self.device)
            if cand.numel() == 0:
                return res
            modes = res["modes"][cand].contiguous()
            scores = (res["counts"] if kernel == "flat" else res["wsum"])[cand].to(torch.float32).contiguous()
            other = TrueKNN(device=self.device.index)
            try:
                other.build(modes)
                kept = other.radius_nms(float(bandwidth if merge_radius is None else merge_radius), scores=scores, want_cover=False)["idx"]
                order = torch.sort(scores[kept], descending=True, stable=True).indices  # (kept ascends by candidate row)
                res["centers"], res["scores"] = modes[kept[order]].contiguous(), scores[kept[order]]
                other.build(res["centers"])
                if cluster_all:
                    near = other.knn(points, k=1, want_dist=False)["idx"]
                else:
                    near = other.radius_knn(points, 1, radius=float(bandwidth), want_dist=False)["idx"]
                res["labels"] = near[:, 0].to(torch.int64)
            finally:
                other.close()
        return res

    def _is_batched(self):
        """Whether the engine's tree is a batched one (tknnBatchLayout answers for those only)."""
        nb = ctypes.c_int32(0)
        with self._torch.cuda.device(self.device):
            return _batch_lib.load().tknnBatchLayout(self._h, ctypes.byref(nb), None, None, self._stream()) == 0

    def _nan_count(self):
        """The built points with a NaN coordinate (tknnExportTreeEx with no array asked for)."""
        x = _lib.TreeExport()
        with self._torch.cuda.device(self.device):
            _lib.check(self._lib.tknnExportTreeEx(self._h, ctypes.byref(x), self._stream()))
        return int(x.nan_count)

    def segment_min(self, segment, value, out):
        """out[segment[i]] = min(out[segment[i]], value[i]) for segment[i] >= 0, in place (tknnSegmentMin): ``segment`` (n,)
        int32, ``value`` (n,) int64, ``out`` (m,) int64 preset by the caller, all on the engine's device."""
        torch = self._torch
        if segment.dtype != torch.int32 or value.dtype != torch.int64 or out.dtype != torch.int64 or segment.shape != value.shape:
            raise ValueError("segment_min: int32 segments, int64 values of the same shape, int64 out")
        with torch.cuda.device(self.device):
            segment, value = segment.contiguous(), value.contiguous()
            _lib.check(self._lib.tknnSegmentMin(self._h, ctypes.c_void_p(segment.data_ptr()), ctypes.c_void_p(value.data_ptr()), int(segment.numel()),
                                                ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out

    def export_tree(self):
        """Host copies of the LBVH for tests: nodes (n-1,8) uint32 view, ropes, prim ids."""
        torch = self._torch
        n = self.n
        nodes = np.zeros((max(n - 1, 1), 8), np.uint32)
        rope_node = np.zeros(max(n - 1, 1), np.int32)
        rope_leaf = np.zeros(n, np.int32)
        prim = np.zeros(n, np.int32)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.tknnExportTree(self._h, nodes.ctypes.data, rope_node.ctypes.data,
                                                rope_leaf.ctypes.data, prim.ctypes.data, self._stream()))
        split_owner = np.zeros(max(n - 1, 1), np.int32)
        paths = np.zeros(((n + 63) // 64, 5), np.int32)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.tknnExportTreeTables(self._h, split_owner.ctypes.data, paths.ctypes.data, self._stream()))
        return {"nodes": nodes[: max(n - 1, 0)], "rope_node": rope_node[: max(n - 1, 0)],
                "rope_leaf": rope_leaf, "prim_id": prim, "split_owner": split_owner[: max(n - 1, 0)], "block_paths": paths}

    def export_tree_ex(self, halo=False):
        """Host copies of everything the readers of a point tree rely on (tknnExportTreeEx), for the own tree or, with
        ``halo``, the halo tree: n, curve, nan_count, scene (6,) float32, keys (n,) uint64, points (ceil(n/16)*16 + 16, 4)
        uint32 records x y z id with the sentinels, prim_id, row_slot, nodes (n-1, 8) uint32, rope_node, rope_leaf,
        split_owner, wide_levels, wide_count (6,) int32 and wide_boxes (sum of the counts, 6) float32, level after level."""
        torch = self._torch
        n = self.halo_n if halo else self.n
        blocks = (n + 15) // 16
        arrays = {"keys": np.zeros(n, np.uint64), "points": np.zeros((blocks * 16 + 16, 4), np.uint32), "row_slot": np.zeros(n, np.int32),
                  "wide_boxes": np.zeros((blocks + blocks // 32 + 6, 6), np.float32), "nodes": np.zeros((max(n - 1, 1), 8), np.uint32),
                  "rope_node": np.zeros(max(n - 1, 1), np.int32), "rope_leaf": np.zeros(n, np.int32), "prim_id": np.zeros(n, np.int32),
                  "split_owner": np.zeros(max(n - 1, 1), np.int32)}
        x = _lib.TreeExport()
        x.which = 1 if halo else 0
        x.wide_capacity = len(arrays["wide_boxes"])
        for name, a in arrays.items():
            setattr(x, name, a.ctypes.data)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.tknnExportTreeEx(self._h, ctypes.byref(x), self._stream()))
        if int(x.n) != n:
            raise RuntimeError("export_tree_ex: the tree holds %d points, %d expected" % (x.n, n))
        out = dict(arrays)
        for name in ("nodes", "rope_node", "split_owner"):
            out[name] = arrays[name][: n - 1]
        out["wide_count"] = np.array(list(x.wide_count), np.int32)
        out["wide_boxes"] = arrays["wide_boxes"][: int(out["wide_count"].sum())]
        out.update(n=n, curve=int(x.curve), nan_count=int(x.nan_count), wide_levels=int(x.wide_levels),
                   scene=np.array(list(x.scene), np.float32))
        return out


def debug_box_tree(boxes, refit=None, mode=0, device=None):
    """The builder's box tree over (n, 6) float32 ``boxes`` {lo xyz, hi xyz} without an engine (tknnDebugBoxTree), refitted
    to ``refit`` where given: dict(nodes (n-1, 8) uint32, rope_node, rope_leaf, prim_id, sorted_boxes (n, 6) float32).
    ``mode`` 1 / 2 ask for a refit of no tree / of a point tree, which raises TknnError (TKNN_E_STATE)."""
    import torch

    lib = _lib.load()
    if not torch.cuda.is_available():
        raise RuntimeError("debug_box_tree needs an MI355X: no GPU is visible and there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    boxes = np.ascontiguousarray(boxes, np.float32)
    n = len(boxes)
    if boxes.shape != (n, 6) or (refit is not None and np.shape(refit) != (n, 6)):
        raise ValueError("debug_box_tree: boxes (and refit) must be (n, 6)")
    nodes = np.zeros((max(n - 1, 1), 8), np.uint32)
    rope_node = np.zeros(max(n - 1, 1), np.int32)
    rope_leaf, prim = np.zeros(n, np.int32), np.zeros(n, np.int32)
    sorted_boxes = np.zeros((n, 6), np.float32)
    with torch.cuda.device(dev):
        d_boxes = torch.from_numpy(boxes).to(dev)
        d_refit = None if refit is None else torch.from_numpy(np.ascontiguousarray(refit, np.float32)).to(dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.tknnDebugBoxTree(ctypes.c_void_p(d_boxes.data_ptr()), n, None if d_refit is None else ctypes.c_void_p(d_refit.data_ptr()),
                                        int(mode), nodes.ctypes.data, rope_node.ctypes.data, rope_leaf.ctypes.data, prim.ctypes.data,
                                        sorted_boxes.ctypes.data, stream))
    return {"nodes": nodes[: n - 1], "rope_node": rope_node[: n - 1], "rope_leaf": rope_leaf, "prim_id": prim, "sorted_boxes": sorted_boxes}


def _one_shot(points, call):
    """An engine built over ``points`` for the one ``call(engine)``: its results as numpy arrays, and the build's info."""
    eng = TrueKNN()
    try:
        eng.build(points)
        res = {name: (v.cpu().numpy() if hasattr(v, "cpu") else v) for name, v in call(eng).items()}
        res["build_info"] = eng.build_info
        return res
    finally:
        eng.close()


def trueknn(points, k, start_radius, **kw):
    """One-shot helper: build + solve, results as numpy arrays."""
    return _one_shot(points, lambda eng: eng.solve(k, start_radius, **kw))


def trueknn_query(points, queries, k, start_radius, **kw):
    """One-shot helper: build over ``points``, answer for ``queries`` (TrueKNN.query), results as numpy arrays."""
    return _one_shot(points, lambda eng: eng.query(queries, k, start_radius, **kw))


def radius_query(points, queries, radius, **kw):
    """One-shot helper: build over ``points``, the neighbours of ``queries`` within ``radius`` (TrueKNN.radius_query), results
    as numpy arrays."""
    return _one_shot(points, lambda eng: eng.radius_query(queries, radius, **kw))


def radius_knn(points, queries, k, **kw):
    """One-shot helper: build over ``points``, at most ``k`` nearest points within a radius of ``queries`` (TrueKNN.radius_knn),
    results as numpy arrays."""
    return _one_shot(points, lambda eng: eng.radius_knn(queries, k, **kw))


def radius_graph(points, k, radius, loop=False):
    """One-shot helper: for every point of ``points`` its at most ``k`` nearest other points within ``radius`` -- radius_knn with
    the points as their own queries and every point skipped in its own row; with ``loop`` the point itself is an entry (at
    distance 0, where k leaves room).  Results as numpy arrays; entry (i, t) is the edge from idx[i, t] to i."""
    points = pad_to_3d(np.asarray(points, np.float32))
    skip = None if loop else np.arange(len(points), dtype=np.int32)
    return radius_knn(points, points, k, radius=radius, skip_ids=skip)


def knn(points, queries, k, **kw):
    """One-shot helper: build over ``points``, the exact ``k`` nearest points of ``queries`` (TrueKNN.knn), results as numpy
    arrays."""
    return _one_shot(points, lambda eng: eng.knn(queries, k, **kw))


def knn_graph(points, k, loop=False):
    """One-shot helper: for every point of ``points`` its ``k`` nearest other points, exactly -- TrueKNN.knn over the set's own
    points; with ``loop`` the points are queries like any others, so the point itself is an entry, at distance 0.  Results as
    numpy arrays; entry (i, t) is the edge from idx[i, t] to i."""
    points = pad_to_3d(np.asarray(points, np.float32))
    return knn(points, points if loop else None, k)


def emst(points, **kw):
    """One-shot helper: build over ``points``, their Euclidean minimum spanning tree (TrueKNN.emst), results as numpy arrays."""
    return _one_shot(points, lambda eng: eng.emst(**kw))


def mutual_reachability_mst(points, min_samples, **kw):
    """One-shot helper: the minimum spanning tree of ``points`` under the mutual-reachability distance, the input of HDBSCAN's
    linkage step.  A point's core distance is the distance to its ``(min_samples - 1)``-th nearest OTHER point, the last
    column of TrueKNN.knn(k = min_samples - 1) -- sklearn's convention, where a point counts itself; ``min_samples`` = 1 is
    the plain Euclidean tree.  A point with fewer than min_samples - 1 other points in reach has an infinite core distance and
    is in no edge.  Results as numpy arrays, ``core_dist`` among them."""
    min_samples = int(min_samples)
    if min_samples < 1:
        raise ValueError("mutual_reachability_mst: min_samples must be >= 1")

    def call(eng):
        if min_samples == 1:
            return eng.emst(**kw)
        core = eng.knn(k=min_samples - 1)["dist"][:, -1].contiguous()
        return dict(eng.emst(core_dist=core, **kw), core_dist=core)

    return _one_shot(points, call)


def hdbscan(points, min_cluster_size=5, min_samples=None, **kw):
    """One-shot helper: build over ``points`` and cluster them (TrueKNN.hdbscan), results as numpy arrays."""
    return _one_shot(points, lambda eng: eng.hdbscan(min_cluster_size, min_samples, **kw))


def linkage(u, v, w=None, n=None, **kw):
    """One-shot helper: the single-linkage dendrogram of the sorted forest (u, v[, w]) over ``n`` vertices (TrueKNN.linkage; ``n``
    defaults to edges + 1, a spanning tree), results as numpy arrays.  No point set is needed."""
    eng = TrueKNN()
    try:
        res = eng.linkage(np.asarray(u), np.asarray(v), None if w is None else np.asarray(w), len(u) + 1 if n is None else n, **kw)
        return {name: (t.cpu().numpy() if hasattr(t, "cpu") else t) for name, t in res.items()}
    finally:
        eng.close()


def linkage_matrix(result, w=None):
    """scipy's linkage matrix Z of a spanning tree: (left, right, w, size) of ``TrueKNN.linkage`` / ``hdbscan(want_linkage=True,
    want_tree=True)`` stacked as float64 rows; ``w`` defaults to the result's own."""
    w = result["w"] if w is None else w
    cols = [result["left"], result["right"], w, result["size"]]
    return np.stack([np.asarray(c.cpu().numpy() if hasattr(c, "cpu") else c, np.float64) for c in cols], axis=1)


def batch_knn(points, batch_x, queries, batch_y, k, **kw):
    """One-shot helper: build over ``points`` with the labels ``batch_x``, at most ``k`` nearest points of ``queries`` among the
    points that carry their label ``batch_y`` (TrueKNN.batch_knn; torch-cluster's ``knn(x, y, k, batch_x, batch_y)``), results as
    numpy arrays.  ``queries`` and ``batch_y`` None: the points' own rows."""
    eng = TrueKNN()
    try:
        eng.build(points, batch=batch_x)
        res = {name: (v.cpu().numpy() if hasattr(v, "cpu") else v) for name, v in eng.batch_knn(queries, k, batch=batch_y, **kw).items()}
        res["build_info"] = eng.build_info
        return res
    finally:
        eng.close()


def batch_knn_graph(points, batch, k, loop=False):
    """One-shot helper: for every point of ``points`` its ``k`` nearest other points of its own batch, exactly (torch-cluster's
    ``knn_graph(x, k, batch, loop)``); with ``loop`` the points are queries like any others, so the point itself is an entry, at
    distance 0.  Results as numpy arrays; entry (i, t) is the edge from idx[i, t] to i."""
    points = pad_to_3d(np.asarray(points, np.float32))
    return batch_knn(points, batch, points if loop else None, batch if loop else None, k)


def fps(points, batch=None, ratio=0.5, **kw):
    """One-shot helper: farthest point sampling of ``points``, inside each cloud of the labels ``batch`` where given
    (TrueKNN.fps; torch-cluster's ``fps(x, batch, ratio)``): the sampled rows of ``points`` as one flat int64 numpy array, the
    clouds in label order, each cloud's samples in the order chosen.  ``num_samples`` / ``num`` instead of ``ratio``: pass
    ``ratio=None``."""
    eng = TrueKNN()
    try:
        eng.build(points, batch=batch)
        res = eng.fps(ratio=ratio, **kw)
        idx, counts = res["idx"].cpu().numpy(), res["counts"].cpu().numpy()
        return np.concatenate([idx[b, : counts[b]] for b in range(len(counts))] + [np.zeros(0, np.int32)]).astype(np.int64)
    finally:
        eng.close()


def radius_nms(points, radius, scores=None, batch=None, **kw):
    """One-shot helper: build over ``points`` -- with the labels ``batch`` where given, one cloud each -- and keep the points that
    no stronger kept point of their cloud has within ``radius`` (TrueKNN.radius_nms), results as numpy arrays."""
    eng = TrueKNN()
    try:
        eng.build(points, batch=batch)
        return {name: (v.cpu().numpy() if hasattr(v, "cpu") else v) for name, v in eng.radius_nms(radius, scores=scores, **kw).items()}
    finally:
        eng.close()


def radius_reduce(points, queries, radius, ids=None, batch=None, **kw):
    """One-shot helper: build over ``points`` and sum over the points within ``radius`` of each of ``queries`` (None: the points
    themselves) what TrueKNN.radius_reduce sums, results as numpy arrays."""
    eng = TrueKNN()
    try:
        eng.build(points, ids=ids, batch=batch)
        res = eng.radius_reduce(radius, queries=queries, **kw)
        return {name: (v.cpu().numpy() if hasattr(v, "cpu") else v) for name, v in res.items()}
    finally:
        eng.close()


def local_pca(points, queries, radius=None, k=None, ids=None, batch=None, **kw):
    """One-shot helper: build over ``points`` and fit a plane to the neighbourhood of each of ``queries`` (None: the points
    themselves) as TrueKNN.local_pca does, results as numpy arrays."""
    eng = TrueKNN()
    try:
        eng.build(points, ids=ids, batch=batch)
        res = eng.local_pca(radius=radius, k=k, queries=queries, **kw)
        return {name: (v.cpu().numpy() if hasattr(v, "cpu") else v) for name, v in res.items()}
    finally:
        eng.close()


def fpfh(points, radius, normals=None, **kw):
    """One-shot helper: build over ``points`` and describe every point by its FPFH as TrueKNN.fpfh does, results as numpy arrays."""
    return _one_shot(points, lambda eng: eng.fpfh(radius, normals=normals, **kw))


def orient_normals(points, normals, **kw):
    """One-shot helper: build over ``points``, one consistent sign per normal with no viewpoint (TrueKNN.orient_normals), results as
    numpy arrays."""
    return _one_shot(points, lambda eng: eng.orient_normals(normals, **kw))


def segment_plane(points, distance_threshold, **kw):
    """One-shot helper: build over ``points`` and take its dominant plane (TrueKNN.segment_plane): (plane, rows) as numpy arrays, or
    with ``return_info=True`` the dict, its tensors as numpy arrays."""
    eng = TrueKNN()
    try:
        eng.build(points)
        res = eng.segment_plane(distance_threshold, **kw)
        if isinstance(res, dict):
            return {name: (v.cpu().numpy() if hasattr(v, "cpu") else v) for name, v in res.items()}
        return tuple(v.cpu().numpy() for v in res)
    finally:
        eng.close()


def icp(target, source, max_dist, **kw):
    """One-shot helper: build over ``target`` and register ``source`` to it (TrueKNN.icp), results as numpy arrays."""
    return _one_shot(target, lambda eng: eng.icp(source, max_dist, **kw))


def _treeless(call):
    """An engine without a tree for the one ``call(engine)``: its results as numpy arrays."""
    eng = TrueKNN()
    try:
        return {name: (t.cpu().numpy() if hasattr(t, "cpu") else t) for name, t in call(eng).items()}
    finally:
        eng.close()


def match_features(source_feat, target_feat, **kw):
    """One-shot helper: match the descriptor rows (TrueKNN.match_features), results as numpy arrays.  No point set is needed."""
    return _treeless(lambda eng: eng.match_features(np.asarray(source_feat), np.asarray(target_feat), **kw))


def ransac(source, target, pairs, max_dist, **kw):
    """One-shot helper: RANSAC over the correspondences (TrueKNN.ransac), results as numpy arrays.  No tree is built."""
    return _treeless(lambda eng: eng.ransac(np.asarray(source, dtype=np.float32), np.asarray(target, dtype=np.float32), np.asarray(pairs), max_dist, **kw))


def voxel_down_sample(points, voxel_size, **kw):
    """One-shot helper: one point per occupied grid cell of edge ``voxel_size``, per cloud of the labels ``batch`` where given
    (TrueKNN.voxel_down_sample), results as numpy arrays.  No tree is built."""
    return _treeless(lambda eng: eng.voxel_down_sample(pad_to_3d(np.asarray(points, np.float32)), voxel_size, **kw))


def global_registration(target, source, feature_radius, max_dist, normal_k=16, mutual=True, icp=True, target_viewpoint=None, source_viewpoint=None,
                        voxel_size=None, **kw):
    """Registration of two unaligned clouds, on the device from end to end: an engine per cloud, ``fpfh(feature_radius,
    normal_k=normal_k)`` on both, ``match_features(mutual=mutual)``, ``ransac(max_dist, **kw)`` and, with ``icp``,
    ``icp(max_dist, init=...)`` on the target's engine.  An FPFH is not invariant under a flip of the normals, and a normal
    without a viewpoint takes its sign from its largest component, which a rotation of the cloud changes: give each cloud the
    position it was seen from (``target_viewpoint``, ``source_viewpoint``, each in its own frame) and its normals are turned
    towards it (``normals(k=normal_k, viewpoint=...)``) before the FPFH.  Returns dict(ransac, ransac_eval, pairs (c,2) numpy,
    match_info[, icp, icp_eval], transform): the results of the calls, and ``evaluate_registration`` of each transform on the full
    clouds; transform: ICP's with ``icp``, else RANSAC's.
    ``voxel_size``: both clouds are first reduced to the centroids of a voxel grid of that edge (``voxel_down_sample``); normals,
    FPFH, matching and RANSAC run on those -- ``pairs`` then names their rows, and ``target_down``, ``source_down`` are the
    numbers of points left --, ICP and both evaluations on the full clouds.  None: nothing is reduced."""
    et, es = TrueKNN(), TrueKNN()
    if voxel_size is not None:
        ed, esd = TrueKNN(), TrueKNN()  # the engines of the reduced clouds; et holds the full target for ICP and the evaluations

    def describe(eng, viewpoint):
        if viewpoint is None:
            return eng.fpfh(feature_radius, normal_k=normal_k)["fpfh"]
        return eng.fpfh(feature_radius, normals=eng.normals(k=normal_k, viewpoint=viewpoint)["normals"])["fpfh"]

    try:
        et.build(target)
        src, tgt = es._queries(source, "global_registration"), et._queries(target, "global_registration")
        if voxel_size is None:
            es.build(source)
            ft, fs = describe(et, target_viewpoint), describe(es, source_viewpoint)
            src_few, tgt_few = src, tgt
        else:
            tgt_few = ed.voxel_down_sample(tgt, voxel_size)["points"].contiguous()
            src_few = esd.voxel_down_sample(src, voxel_size)["points"].contiguous()
            ed.build(tgt_few)
            esd.build(src_few)
            ft, fs = describe(ed, target_viewpoint), describe(esd, source_viewpoint)
        match = es.match_features(fs, ft, mutual=mutual)
        rs = es.ransac(src_few, tgt_few, match["pairs"], max_dist, **kw)
        out = {"ransac": rs, "pairs": match["pairs"].cpu().numpy(), "match_info": match["info"], "transform": rs["transform"],
               "ransac_eval": et.evaluate_registration(src, max_dist, init=rs["transform"])}
        if voxel_size is not None:
            out["target_down"], out["source_down"] = int(tgt_few.shape[0]), int(src_few.shape[0])
        if icp:
            out["icp"] = et.icp(src, max_dist, init=rs["transform"])
            out["transform"] = out["icp"]["transform"]
            out["icp_eval"] = et.evaluate_registration(src, max_dist, init=out["transform"])
        return out
    finally:
        et.close()
        es.close()
        if voxel_size is not None:
            ed.close()
            esd.close()


def bin_seeds(points, bin_size, min_bin_freq=1):
    """The seeds sklearn's ``get_bin_seeds`` gives, made on the device: the points (numpy (n,2|3) or a float32 (n,3) CUDA tensor;
    rows with a coordinate that is not finite are left out) are binned onto the grid round(p / bin_size) in fp32, the bins with at
    least ``min_bin_freq`` points are kept (torch.unique on a packed int64 key, with counts), and a seed is its bin times
    ``bin_size``.  Returns a float32 (s,3) tensor on the points' device, the seeds in ascending (x, y, z) bin order: the result
    does not depend on the order of the points."""
    import torch

    if isinstance(points, np.ndarray):
        points = torch.from_numpy(pad_to_3d(np.asarray(points, np.float32))).to("cuda")
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or not points.is_cuda:
        raise ValueError("bin_seeds: points must be float32 (n,3) on the GPU")
    if not float(bin_size) > 0:
        raise ValueError("bin_seeds: bin_size must be > 0")
    size = torch.tensor(float(bin_size), dtype=torch.float32, device=points.device)  # (a tensor: a true division, not a reciprocal)
    points = points[torch.isfinite(points).all(dim=1)]
    if points.shape[0] == 0:
        return torch.empty((0, 3), dtype=torch.float32, device=points.device)
    bins = torch.round(points / size).to(torch.int64)
    lo = bins.min(dim=0).values
    span = (bins.max(dim=0).values - lo + 1).tolist()
    if span[0] * span[1] * span[2] >= 2 ** 62:
        raise ValueError("bin_seeds: the grid of bins does not fit an int64 key; choose a larger bin_size")
    rel = bins - lo
    key = (rel[:, 0] * span[1] + rel[:, 1]) * span[2] + rel[:, 2]
    uniq, freq = torch.unique(key, return_counts=True)  # ascending
    uniq = uniq[freq >= int(min_bin_freq)]
    cell = torch.stack([uniq // (span[1] * span[2]), (uniq // span[2]) % span[1], uniq % span[2]], dim=1) + lo
    return (cell.to(torch.float32) * size).contiguous()


def mean_shift(points, bandwidth, seeds=None, **kw):
    """One-shot helper: build over ``points`` and cluster them by mean shift from ``seeds`` (None: the points themselves;
    ``bin_seeds(points, bandwidth)`` for sklearn's bin_seeding) as TrueKNN.mean_shift does, results as numpy arrays."""
    points = pad_to_3d(np.asarray(points, np.float32))
    return _one_shot(points, lambda eng: eng.mean_shift(bandwidth, seeds=seeds, points=points, **kw))


def dbscan_query(points, queries, eps, min_pts):
    """One-shot helper: cluster ``points`` (TrueKNN.dbscan), then label ``queries`` against that clustering
    (TrueKNN.dbscan_query).  dict(labels (m,), counts (m,), point_labels (n,), point_core (n,), clusters) as numpy arrays."""
    eng = TrueKNN()
    try:
        eng.build(points)
        c = eng.dbscan(eps, min_pts)
        r = eng.dbscan_query(queries, eps, c["labels"], core=c["core"], want_counts=True)
        return {"labels": r["labels"].cpu().numpy(), "counts": r["counts"].cpu().numpy(), "point_labels": c["labels"].cpu().numpy(),
                "point_core": c["core"].cpu().numpy(), "clusters": c["info"]["clusters"], "info": r["info"]}
    finally:
        eng.close()
