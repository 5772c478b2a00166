"""Multi-GPU TrueKNN: Morton tiles + halo exchange.

The reference has no multi-GPU path for this workload (it replicates every buffer and the BVH on
every device and pins the sample to one GPU, owl/RayGen.cpp:150-200, hostCode.cpp:141).  Here the
path shards naturally -- queries are independent -- with ONE real exchange step:

  * the global point set is cut into W contiguous ranges of the 63-bit Morton order with equal
    counts (splitters from a sorted sample); rank g owns the queries and result rows of tile g and
    keeps an LBVH over its own points (built once, like the single-GPU build); because a Morton
    range is not spatially compact (Z-curve jumps), a tile is described by the bounding boxes of its
    level-2 Morton cells (<= 64 compact boxes), not by one box;
  * per solve, every rank sends each peer the points of its tile that lie within the halo radius of
    one of the peer's cell boxes -- exactly the foreign points that can be box candidates of the
    peer's queries (the reference's candidate test is an L-inf box) -- as one
    point-to-point exchange (RCCL send/recv over xGMI; a few MB per pair, latency-bound);
  * the engine searches own tree + halo tree; a query's row is exact as soon as its final radius
    does not exceed the halo radius, which one 8-byte all-reduce checks; stragglers double the halo
    radius and go again.  Neighbour indices are global, so rows equal the single-GPU result.

One process per GPU (torch.distributed, backend "nccl" = RCCL on ROCm); with backend "gloo" the
same code runs with host-staged messages (CPU tests, or several ranks sharing one GPU).

``_Comm._exchange_capped`` is the fixed-capacity exchange; ``exchange_rows`` (rows on hand) and
``exchange_fixed`` (messages selected in place) build its messages.  ``ShardedTrueKNN.solve`` loops over
``_select``, ``_interior_solve``, ``_exchange``, ``_engine_step``, ``_anyone_left`` around one ``_SolveState``.
"""
import contextlib
import os
import threading
import time

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, datasets


def morton63(points, lo, extent):
    """63-bit Morton codes (21 bits per axis, x most significant) of float32 points, as int64."""
    scale = 2097151.0 / extent if extent > 0 else 0.0
    q = ((points.double() - lo.double()) * scale).clamp_(0, 2097151).long()

    def spread(v):
        v = v & 0x1FFFFF
        v = (v | (v << 32)) & 0x1F00000000FFFF
        v = (v | (v << 16)) & 0x1F0000FF0000FF
        v = (v | (v << 8)) & 0x100F00F00F00F00F
        v = (v | (v << 4)) & 0x10C30C30C30C30C3
        v = (v | (v << 2)) & 0x1249249249249249
        return v

    return (spread(q[:, 0]) << 2) | (spread(q[:, 1]) << 1) | spread(q[:, 2])


def sample_positions(count, samples, device):
    """`samples` evenly spaced positions in [0, count-1], first and last included, in exact integer
    arithmetic (a float32 linspace rounds its end point up to `count` once count > 2**24: an
    out-of-bounds gather on tiles of 50 M points)."""
    last = max(int(count) - 1, 0)
    steps = torch.arange(samples, dtype=torch.int64, device=device)
    return (steps * last) // max(samples - 1, 1)


def _count_cells(count):
    """A row count as the two header cells of a fixed-capacity message: low 24 bits, the rest (float32 holds integers
    below 2**24 exactly).  TrueKNN.halo_select_fixed writes the same cells on the device."""
    return float(count % (1 << 24)), float(count >> 24)


def _count_of_cells(low, high):
    """The row count two header cells carry (see _count_cells)."""
    return int(low) + (int(high) << 24)


_BIG = torch.iinfo(torch.int64).max  # "no label yet" in the label propagation of dbscan


def _row_ids(rows):
    """the global ids of 16-byte wire rows x y z id-bits"""
    return rows[:, 3].contiguous().view(torch.int32)


class _PhaseClock:
    """Wall time per named phase of a solve / dbscan call.  Only with ``on`` (TKNN_SHARD_PROFILE, bench.py's instrumented
    steps) does a lap synchronise the device and count; otherwise it costs a clock read."""

    def __init__(self, names, device, on):
        self.ms, self.device, self.on = dict.fromkeys(names, 0.0), device, on
        self.restart()

    def restart(self):
        self.t = time.perf_counter()

    def lap(self, name):
        if self.on:
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            self.ms[name] += (time.perf_counter() - self.t) * 1e3
        self.restart()


class _Comm:
    """The three collectives the path needs, on device tensors (nccl) or host-staged (gloo)."""

    def __init__(self, group=None):
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.staged = dist.get_backend(group) != "nccl"
        self._caps = {}  # (tag, "in" | "out") -> rows per peer the next fixed-capacity exchange under that tag holds

    def _wire(self, t):
        return t.cpu() if self.staged and t.is_cuda else t

    def all_reduce(self, t, op):
        w = self._wire(t)
        dist.all_reduce(w, op=op, group=self.group)
        if w is not t:
            t.copy_(w)
        return t

    def all_gather(self, t):
        w = self._wire(t.contiguous())
        out = [torch.empty_like(w) for _ in range(self.world)]
        dist.all_gather(out, w, group=self.group)
        return torch.stack(out).to(t.device)

    def _recv_buffer(self, rows, width, dtype, device):
        """where a message of ``rows`` rows lands: on the host when messages are staged, else on ``device``"""
        return torch.empty((int(rows), width), dtype=dtype, device="cpu" if self.staged else device)

    def _transfer(self, sends, recvs):
        """ONE batched send/recv, waited for: ``sends`` {peer: tensor}, ``recvs`` {peer: buffer to fill}."""
        ops = []
        for p in range(self.world):
            if p in sends:
                ops.append(dist.P2POp(dist.isend, self._wire(sends[p]), p, group=self.group))
            if p in recvs:
                ops.append(dist.P2POp(dist.irecv, recvs[p], p, group=self.group))
        if ops:  # (no ops: nothing to wait for)
            for req in dist.batch_isend_irecv(ops):
                req.wait()

    def _exchange_exact(self, sends, expect, width, dtype, device):
        """Exact-size messages whose sizes both ends know: ``sends`` {peer: rows}, ``expect`` {peer: rows that arrive}; an
        empty block does not travel.  Returns {peer: the rows received, on ``device``}."""
        recv = {p: self._recv_buffer(c, width, dtype, device) for p, c in expect.items()}
        self._transfer({p: r.contiguous() for p, r in sends.items() if len(r)}, {p: b for p, b in recv.items() if len(b)})
        return {p: b.to(device) for p, b in recv.items()}

    def _exchange_capped(self, tag, messages, counts_out, exact_blocks, width, dtype, device):
        """The fixed-capacity exchange under ``tag``: ``messages[p]`` (a header row with my count + cap_out[p] rows) goes to peer
        p, cap_in[p] + 1 rows arrive from it, and ONE host read brings the counts of what arrived -- and my own, when
        ``counts_out`` is a device tensor and not a host list.  A pair whose rows outgrew its capacity (both ends see it: the
        sender by its count, the receiver by the header) goes through exact-size messages once more; ``exact_blocks()`` then
        returns my exact rows per peer.  Capacities: what both ends remember of the pair's exchanges under the tag (_remember).
        Returns (rows received per source, rows sent per destination), None at my own rank."""
        world, me = self.world, self.rank
        cap_in, cap_out = self._caps[(tag, "in")], self._caps[(tag, "out")]
        peers = [p for p in range(world) if p != me]
        recv = {p: self._recv_buffer(cap_in[p] + 1, width, dtype, device) for p in peers}
        self._transfer({p: messages[p] for p in peers}, recv)
        cells = [recv[p][0, :2] for p in peers]
        if torch.is_tensor(counts_out):  # my counts join the read: first in it, as float64 like the cells then
            cells = [counts_out.to(cells[0].device if peers else counts_out.device).double()] + [c.double() for c in cells]
        flat = torch.cat(cells).tolist() if cells else []  # the step's one host round trip
        if torch.is_tensor(counts_out):
            counts_out, flat = [int(c) for c in flat[:world]], flat[world:]
        counts_in = [0] * world
        for j, p in enumerate(peers):
            counts_in[p] = _count_of_cells(flat[2 * j], flat[2 * j + 1])
        late_in = {p: counts_in[p] for p in peers if counts_in[p] > cap_in[p]}
        late_out = [p for p in peers if counts_out[p] > cap_out[p]]
        got, sent = [None] * world, [None] * world
        for p in peers:
            if p not in late_in:
                got[p] = recv[p][1:1 + counts_in[p]].to(device)
            sent[p] = messages[p][1:1 + min(counts_out[p], cap_out[p])]
        if late_in or late_out:
            exact = exact_blocks() if late_out else None
            for p in late_out:
                sent[p] = exact[p]
            for p, rows in self._exchange_exact({p: exact[p] for p in late_out}, late_in, width, dtype, device).items():
                got[p] = rows
        self._remember(tag, counts_in, counts_out)
        return got, sent

    def exchange_rows(self, rows_per_peer, width, dtype, device, tag=None, counts_in=None):
        """all-to-all-v of 2-D row blocks: rows_per_peer[p] goes to rank p; returns the list of
        blocks received (index = source rank).

        Without ``tag``: counts first (an all-gather and a host round trip), then one batched
        send/recv of exactly those rows.  With ``counts_in`` (rows per source, known to the caller):
        just that send/recv.  With ``tag`` (the per-step halo exchange): ONE batched
        send/recv of fixed-capacity, zero-filled messages whose first row carries the count
        (_exchange_capped); the first exchange under a tag goes the counts-first way and teaches
        both ends of every pair the capacity (x 1.25 + 64 rows)."""
        world, me = self.world, self.rank
        if world == 1:  # nobody to exchange with (and no count to agree on)
            return [rows_per_peer[0]]
        counts_out = [len(r) for r in rows_per_peer]
        if tag is not None and dtype == torch.float32 and self.has_caps(tag):
            cap_out = self._caps[(tag, "out")]
            messages = [None if p == me else self._message(rows, cap_out[p], width) for p, rows in enumerate(rows_per_peer)]
            got, _ = self._exchange_capped(tag, messages, counts_out, lambda: rows_per_peer, width, dtype, device)
            got[me] = rows_per_peer[me]
            return got
        if counts_in is None:
            counts = torch.tensor(counts_out, dtype=torch.int64, device=device)
            counts_in = self.all_gather(counts)[:, me].tolist()  # [src] rows coming from src
        # (else: the caller knows what arrives -- the answers to rows it has sent, say -- and no count travels)
        got = self._exchange_exact({p: r for p, r in enumerate(rows_per_peer) if p != me},
                                   {p: c for p, c in enumerate(counts_in) if p != me}, width, dtype, device)
        if tag is not None and dtype == torch.float32:
            self._remember(tag, [int(c) for c in counts_in], counts_out)
        return [rows_per_peer[me].to(device) if p == me else got[p] for p in range(world)]

    @staticmethod
    def _message(rows, cap, width):
        """a zero-filled fixed-capacity message: the count of ``rows`` in its header row, then the first ``cap`` of them"""
        m = torch.zeros((cap + 1, width), dtype=rows.dtype, device=rows.device)
        m[0, 0], m[0, 1] = _count_cells(len(rows))
        take = min(len(rows), cap)
        if take:
            m[1:1 + take] = rows[:take]
        return m

    def has_caps(self, tag):
        return (tag, "in") in self._caps

    def caps_out(self, tag):
        return list(self._caps[(tag, "out")])

    def exchange_fixed(self, messages, starts, counts_dev, tag, device, exact_blocks):
        """The tagged exchange for rows that were SELECTED straight into fixed-capacity messages (TrueKNN.halo_select_fixed): the
        messages leave as they are, the headers of what arrives and my own counts come to the host in ONE read -- the step's only
        round trip before the solve (the two-pass selection had one of its own).  A pair whose rows outgrew its capacity goes
        through exact-size messages once more; ``exact_blocks()`` then returns the per-peer rows the two-pass selection gives.
        Rows past the count in a selected message are unspecified device memory and travel as they are.
        Returns (rows received per source, rows sent per destination)."""
        cap_out = self._caps[(tag, "out")]
        per_peer = [messages[s: s + cap_out[p] + 1] for p, s in enumerate(starts)]
        got, sent = self._exchange_capped(tag, per_peer, counts_dev, exact_blocks, 4, torch.float32, device)
        got[self.rank] = sent[self.rank] = messages[:0]
        return got, sent

    def _remember(self, tag, counts_in, counts_out):
        """capacities of the next exchange under ``tag``: both ends of a pair derive the same number from the same count"""
        grow = lambda c: int(c) + int(c) // 4 + 64  # noqa: E731
        old_in, old_out = self._caps.get((tag, "in")), self._caps.get((tag, "out"))
        self._caps[(tag, "in")] = [max(grow(c), old_in[p] if old_in else 0) for p, c in enumerate(counts_in)]
        self._caps[(tag, "out")] = [max(grow(c), old_out[p] if old_out else 0) for p, c in enumerate(counts_out)]


class _SolveState:
    """What one ShardedTrueKNN.solve carries from step to step."""

    def __init__(self, world):
        self.halo = None            # every foreign row received so far (the halo tree's points)
        self.held = [None] * world  # ids of my rows each peer holds already
        self.round_halo = []        # rows received per exchange; its length is the number of exchanges
        self.one_pass = False       # the first exchange selected its rows straight into fixed-capacity messages
        self.overlapped = False     # the interior queries were solved beside the first exchange
        self.res = None             # the last engine result; None: the first step is still to come

    def travelled(self, peer, rows):
        """``rows`` of mine went to ``peer``: it holds them from now on, and a straggler round sends only what it lacks"""
        if len(rows):
            self.held[peer] = _row_ids(rows) if self.held[peer] is None else torch.cat([self.held[peer], _row_ids(rows)])


class ShardedTrueKNN:
    """TrueKNN over a point set sharded across the ranks of a process group.

    ``engine_factory(device)`` must return an object with the ``owlraytracing_amd.trueknn.TrueKNN``
    interface (build / set_halo / solve); the default is that class, i.e. the HIP engine.  Tests
    inject a checker-backed stand-in to run the partition / halo / validity logic on CPU ranks.
    """

    CELL_LEVEL = 2   # a tile is described by the boxes of its Morton cells at this level ...
    MAX_CELLS = 64   # ... of which there are at most 8 ** CELL_LEVEL

    def __init__(self, device, kernel=_lib.KERNEL_AUTO, engine_factory=None, group=None, halo_levels=None):
        self.device = torch.device(device)
        self.kernel = kernel
        self.comm = _Comm(group)
        if engine_factory is None:
            from .trueknn import TrueKNN
            engine_factory = lambda dev: TrueKNN(device=dev.index)  # noqa: E731
        self.engine = engine_factory(self.device)
        self._engine_factory = engine_factory
        self.db_engine = None   # second engine over own + halo points (dbscan)
        self._db_cache = None   # (eps, what _db_setup returned for it)
        # first halo radius = start_radius * 2**halo_levels; None: from the density of the set, the level
        # at which a box is expected to hold 32 k points (nearly every query has finished by then, so
        # one exchange and one solve do; stragglers still widen the halo and go again)
        self.halo_levels = halo_levels
        self.extent = None      # (3,) float64 extents of the whole set
        self.points = None      # (m,3) float32 owned points, on self.device
        self.ids = None         # (m,) int32 global ids of the owned points
        self.tile_boxes = None  # (W, MAX_CELLS, 6) float64 on the host: boxes of every rank's Morton cells
        self.cell_boxes = None  # (C,6) my own cells
        self.cell_slices = None  # [(start, end)] of my cells in self.points
        self.n_total = 0
        self.last = None
        self.profile = bool(os.environ.get("TKNN_SHARD_PROFILE"))  # per-phase wall times in info (adds syncs)
        # Opt-in (TKNN_SHARD_OVERLAP=1): solve the queries no foreign point can reach ("interior": not inside any peer's
        # widened cell box) in the own tree while the halo travels and its tree is built; the boundary queries follow
        # with own + halo tree (tknnSolveOptions.phase).  Rows are identical either way (tests).  Off by default: the
        # packet kernel is persistent and fills every CU, so the exchange's own kernels (RCCL send/recv, the halo
        # tree build) queue behind it instead of running beside it, and two launches + two host round trips replace
        # one -- measured with two ranks sharing one MI355X (gloo-staged messages): 12.2 ms per step against 6.5 ms
        # in the serial order.
        self.overlap = os.environ.get("TKNN_SHARD_OVERLAP", "0") == "1"
        self._boundary_marked = False
        self._out = {}

    # ---- one-time distribution -------------------------------------------------------------
    def load_counter_based(self, n_total, seed=0):
        """Every rank generates its slice of the C4-style counter-based uniform set, then tiles."""
        w, r = self.comm.world, self.comm.rank
        lo, hi = n_total * r // w, n_total * (r + 1) // w
        pts = torch.from_numpy(datasets.uniform3d_counter(lo, hi, seed=seed)).to(self.device)
        ids = torch.arange(lo, hi, dtype=torch.int32, device=self.device)
        self.load_points(pts, ids)

    def load_points(self, points, ids):
        """Redistribute (points, global ids) so that rank g holds Morton tile g; build own tree."""
        comm, dev = self.comm, self.device
        if isinstance(points, np.ndarray):
            points = torch.from_numpy(datasets.pad_to_3d(points))
        if isinstance(ids, np.ndarray):
            ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32))
        points, ids = points.to(dev).float().contiguous(), ids.to(dev).int().contiguous()
        big = torch.finfo(torch.float32).max
        lo = points.min(0).values.double() if len(points) else torch.full((3,), big, dtype=torch.float64, device=dev)
        hi = points.max(0).values.double() if len(points) else torch.full((3,), -big, dtype=torch.float64, device=dev)
        comm.all_reduce(lo, dist.ReduceOp.MIN)
        comm.all_reduce(hi, dist.ReduceOp.MAX)
        extent = float((hi - lo).max())
        self.extent = (hi - lo).cpu()
        codes = morton63(points, lo, extent)
        order = torch.argsort(codes)
        codes, points, ids = codes[order], points[order], ids[order]
        # splitters: W-quantiles of the union of per-rank sorted samples
        s = 1024
        pick = sample_positions(len(codes), s, dev)
        sample = codes[pick] if len(codes) else torch.full((s,), 2 ** 62, dtype=torch.int64, device=dev)
        allsamp = comm.all_gather(sample).flatten().sort().values
        cut = torch.tensor([len(allsamp) * (g + 1) // comm.world for g in range(comm.world - 1)], device=dev).long()
        splitters = allsamp[cut] if comm.world > 1 else allsamp[:0]
        dest = torch.searchsorted(splitters, codes, right=True)
        rows = torch.cat([points, ids.view(torch.float32).unsqueeze(1)], dim=1)  # 16-byte rows: x y z id-bits
        blocks = [rows[dest == p] for p in range(comm.world)]
        got = torch.cat(comm.exchange_rows(blocks, 4, torch.float32, dev), dim=0)
        if len(got) == 0:
            raise RuntimeError("rank %d received an empty tile; use fewer ranks for this point set" % comm.rank)
        # keep the tile in Morton order: its cells are then contiguous slices
        mycodes = morton63(got[:, :3], lo, extent)
        order = torch.argsort(mycodes)
        got, mycodes = got[order].contiguous(), mycodes[order]
        self.points = got[:, :3].contiguous()
        self._db_cache = None
        self.ids = got[:, 3].contiguous().view(torch.int32)
        self._rows = got  # 16-byte wire rows: x y z id-bits
        n_local = torch.tensor([len(self.points)], dtype=torch.int64, device=dev)
        self.n_total = int(comm.all_reduce(n_local.clone(), dist.ReduceOp.SUM).item())
        # A Morton range is NOT spatially compact: a tile that ends just past a jump of the Z curve
        # has a bounding box spanning far-apart regions, and "points near the tile's box" would be
        # most of the data set.  So a tile is described by the boxes of its level-2 Morton cells
        # (<= 64 per tile, each inside one cell of the 4x4x4 grid, hence compact).
        cells = mycodes >> (63 - 3 * self.CELL_LEVEL)
        uniq, counts = torch.unique_consecutive(cells, return_counts=True)
        ends = torch.cumsum(counts, 0).tolist()
        starts = [0] + ends[:-1]
        self.cell_slices = list(zip(starts, ends))
        boxes = torch.full((self.MAX_CELLS, 6), float("inf"), dtype=torch.float64, device=dev)
        boxes[:, 3:] = -float("inf")
        for j, (s0, s1) in enumerate(self.cell_slices):
            seg = self.points[s0:s1]
            boxes[j, :3] = seg.min(0).values.double()
            boxes[j, 3:] = seg.max(0).values.double()
        self.cell_boxes = boxes[: len(self.cell_slices)].cpu()
        self.tile_boxes = comm.all_gather(boxes).cpu()  # (W, MAX_CELLS, 6); empty slots are inverted boxes
        self.engine.build(self.points, self.ids)

    # ---- per-solve exchange ---------------------------------------------------------------------
    @staticmethod
    def _reach(radius):
        """How far beyond a peer's cell box a point of mine can lie and still be a box candidate of a query at ``radius``:
        the radius and a relative 1e-5 (_widen adds an ulp-of-coordinate margin and rounds outward)."""
        return float(radius) * (1.0 + 1e-5) + 1e-30

    def _halo_blocks(self, radius):
        """For each peer, the rows of my tile within `radius` (L-inf) of any of the peer's cell boxes:
        exactly the foreign points that can be box candidates of the peer's queries.

        Per peer: my cells whose box meets one of the peer's widened boxes are found on the host
        (<= 64 x 64 tiny tests); only those slices are tested point by point, in float32 against
        boxes widened in float64 (radius, a relative 1e-5, an ulp-of-coordinate margin) and rounded
        OUTWARD, so the selection can only err on the side of sending a point too many."""
        comm, dev = self.comm, self.device
        rows = self._rows
        if hasattr(self.engine, "halo_select"):
            # the engine's kernels do the selection on its own Morton-sorted points: widened peer boxes
            # in, per-peer contiguous wire rows out (tknnHaloSelect)
            boxes, owner = self._peer_boxes(self._reach(radius))
            if boxes is None:
                return [rows[:0] for _ in range(comm.world)]
            rows, counts = self.engine.halo_select(boxes, owner, comm.world)
            self._boundary_marked = True  # the count pass has marked my points inside a peer's box: my boundary queries
            return list(torch.split(rows, counts))
        blocks = [rows[:0] for _ in range(comm.world)]
        mine = self.cell_boxes  # (C,6) float64, host
        for peer, lo64, hi64, lo, hi in self._peer_cells(self._reach(radius)):
            # which of my cells meet any widened peer box (host)
            meet = ((mine[:, None, :3] <= hi64[None]) & (mine[:, None, 3:] >= lo64[None])).all(dim=2)  # (C,P)
            lo, hi = lo.to(dev), hi.to(dev)
            picked = []
            for c, (s0, s1) in enumerate(self.cell_slices):
                which = torch.nonzero(meet[c]).flatten()
                if len(which) == 0:
                    continue
                seg = self.points[s0:s1]
                blo, bhi = lo[which.to(dev)], hi[which.to(dev)]
                inside = ((seg[:, None, :] >= blo[None]) & (seg[:, None, :] <= bhi[None])).all(dim=2).any(dim=1)
                picked.append(rows[s0:s1][inside])
            if picked:
                blocks[peer] = torch.cat(picked, dim=0)
        return blocks

    def _peer_cells(self, reach):
        """(peer, lo64, hi64, lo, hi) for every peer that has cells: its cell boxes widened by ``reach`` in float64, and the
        float32 boxes that contain those (_widen)"""
        for peer in range(self.comm.world):
            pb = self.tile_boxes[peer]
            pb = pb[pb[:, 0] <= pb[:, 3]]  # drop empty slots
            if peer != self.comm.rank and len(pb):
                yield (peer,) + self._widen(pb, reach)

    def _peer_boxes(self, reach):
        """(boxes (m,6) float32, owner (m,) int32) of every peer's Morton cells widened by ``reach``, or (None, None)"""
        boxes, owner = [], []
        for peer, _, _, lo, hi in self._peer_cells(reach):
            boxes.append(torch.cat([lo, hi], dim=1))
            owner.append(torch.full((len(lo),), peer, dtype=torch.int32))
        if not boxes:
            return None, None
        return torch.cat(boxes), torch.cat(owner)

    @staticmethod
    def _widen(pb, reach):
        """pb (float64 cell boxes) widened by `reach` and a relative 1e-6: (lo64, hi64, lo, hi), the last two float32 boxes
        containing the first two, rounded OUTWARD: the selection can only err on the side of sending a point too many."""
        mag = pb.abs().max(dim=1, keepdim=True).values
        lo64, hi64 = pb[:, :3] - reach - 1e-6 * mag, pb[:, 3:] + reach + 1e-6 * mag
        lo, hi = lo64.float(), hi64.float()
        lo = torch.where(lo.double() > lo64, torch.nextafter(lo, torch.full_like(lo, -float("inf"))), lo)
        hi = torch.where(hi.double() < hi64, torch.nextafter(hi, torch.full_like(hi, float("inf"))), hi)
        return lo64, hi64, lo, hi

    @staticmethod
    def _merge_infos(a, b, levels_counted_twice):
        """info of two engine calls that together are one solve (interior + boundary queries; a solve and the re-solve of
        the queries it left unfinished, whose ``levels_counted_twice`` active levels the first call has counted already)"""
        merged = dict(b)
        for key in ("total_intersections", "total_active_rounds", "node_tests", "point_tests", "tie_rows", "tie_rows_left", "solve_ms", "tie_ms"):
            merged[key] = a[key] + b[key]
        merged["total_active_rounds"] -= levels_counted_twice
        merged["unfinished"] = b["unfinished"] if levels_counted_twice else a["unfinished"] + b["unfinished"]
        merged["rounds"] = max(a["rounds"], b["rounds"])
        merged["final_radius"] = max(a["final_radius"], b["final_radius"])
        merged["dominant_kernel_launches"] = a["dominant_kernel_launches"] + b["dominant_kernel_launches"]
        merged["dominant_kernel_ms"] = ((a["dominant_kernel_ms"] * a["dominant_kernel_launches"] + b["dominant_kernel_ms"] * b["dominant_kernel_launches"])
                                        / max(merged["dominant_kernel_launches"], 1))
        return merged

    def _first_halo_level(self, k, r0):
        """The radius level the first halo covers: ``halo_levels``, or the level (<= 6) the density of the set suggests."""
        if self.halo_levels is not None:
            return self.halo_levels
        ext = [float(e) for e in self.extent if float(e) > 0]
        measure = float(np.prod(ext)) if ext else 0.0
        level = 0
        if measure > 0:
            density = self.n_total / measure
            while level < 6 and density * (2.0 * float(r0) * 2 ** level) ** len(ext) < 32.0 * k:
                level += 1
        return level

    @staticmethod
    def _halo_radius(r0, level):
        """The engine's radius at ``level``: r0 doubled ``level`` times in float32, bit for bit what its rounds use."""
        radius = np.float32(r0)
        for _ in range(level):
            radius = np.float32(radius * np.float32(2))
        return radius

    def _select(self, st, tag, halo_radius):
        """My rows for every peer at ``halo_radius``: (None, fixed selection) in a step's usual form (round 4) -- both ends of
        every pair remember how much travelled under ``tag``, so the rows are selected straight into messages of that capacity,
        one pass and no host round trip of its own --, else (per-peer blocks, None): the first exchange under a tag, engines
        without the one-pass selection, and the straggler rounds, whose blocks hold only the SHELL a peer does not hold yet
        (SURVEY 8e).  ``_boundary_marked`` says afterwards whether the engine has marked my boundary queries."""
        comm, first = self.comm, st.res is None
        self._boundary_marked = False
        if (first and comm.world > 1 and comm.has_caps(tag) and hasattr(self.engine, "halo_select_fixed")
                and not (self.overlap and getattr(self.engine, "supports_phases", False))):
            boxes, owner = self._peer_boxes(self._reach(halo_radius))
            if boxes is not None:
                caps = [0 if p == comm.rank else c for p, c in enumerate(comm.caps_out(tag))]
                selection = self.engine.halo_select_fixed(boxes, owner, comm.world, caps)
                self._boundary_marked = st.one_pass = True
                return None, selection
        blocks = self._halo_blocks(halo_radius)
        for p in range(comm.world):
            if p == comm.rank or not len(blocks[p]):
                continue
            if not first and st.held[p] is not None:
                blocks[p] = blocks[p][~torch.isin(_row_ids(blocks[p]), st.held[p])]
            st.travelled(p, blocks[p])
        return blocks, None

    @contextlib.contextmanager
    def _interior_solve(self, st, k, r0, want_fb, solve_kw):
        """Around the first exchange, with TKNN_SHARD_OVERLAP=1: the interior queries (own tree only) are solved on a stream
        and a host thread of their own -- the engine call returns when its kernels are done, so the thread that drives the
        exchange cannot issue it.  Yields None without an interior solve, else a dict that holds ``res`` and ``ms`` once the
        block is left.  The worker uses self.engine: it is joined whatever the block raises, and what it raised
        itself is raised again on the driving thread."""
        dev = self.device
        if not (st.res is None and self.overlap and self._boundary_marked and getattr(self.engine, "supports_phases", False)
                and dev.type == "cuda" and k <= 64 and self.kernel in (_lib.KERNEL_AUTO, _lib.KERNEL_TEAM)):
            yield None
            return
        st.overlapped = True
        n_own = len(self.points)
        if self._out.get("idx") is None or tuple(self._out["idx"].shape) != (n_own, k):
            self._out = {"idx": torch.empty((n_own, k), dtype=torch.int32, device=dev),
                         "dist": torch.empty((n_own, k), dtype=torch.float32, device=dev),
                         "intersections": torch.empty((n_own,), dtype=torch.int64, device=dev),
                         "levels": torch.empty((n_own,), dtype=torch.int32, device=dev)}
        if want_fb and self._out.get("fb") is None:
            self._out["fb"] = torch.empty((n_own * k * 24,), dtype=torch.uint8, device=dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        self.engine.set_halo(None, None)
        interior = {}

        def run_interior():
            try:
                interior["res"] = self.engine.solve(k, float(r0), out=self._out, phase=1, stream=side, **solve_kw)
            except BaseException as e:  # re-raised on the driving thread
                interior["error"] = e

        worker = threading.Thread(target=run_interior, name="tknn-interior")
        t0 = time.perf_counter()
        worker.start()
        try:
            yield interior
        finally:
            worker.join()
        if "error" in interior:
            raise interior["error"]
        interior["ms"] = (time.perf_counter() - t0) * 1e3

    def _exchange(self, st, tag, blocks, selection, halo_radius, clock):
        """One point-to-point exchange of what _select chose (tagged: one host round trip once a first exchange at this
        radius level has taught the capacities), then the halo tree over every foreign row received so far."""
        comm, dev = self.comm, self.device
        if selection is not None:
            got, went = comm.exchange_fixed(*selection, tag, dev, lambda: self._halo_blocks(halo_radius))
            for p in range(comm.world):
                if p != comm.rank:
                    st.travelled(p, went[p])
        else:
            got = comm.exchange_rows(blocks, 4, torch.float32, dev, tag=tag)
        got[comm.rank] = got[comm.rank][:0]
        new_rows = torch.cat(got, dim=0)
        clock.lap("exchange")
        st.round_halo.append(int(len(new_rows)))
        st.halo = new_rows if st.halo is None else torch.cat([st.halo, new_rows], dim=0)
        self.engine.set_halo(st.halo[:, :3].contiguous(), _row_ids(st.halo))
        clock.lap("halo_build")

    def _engine_step(self, st, k, r0, level, interior, solve_kw):
        """The engine call of a step; ``st.res`` then holds every row and the info of the whole solve so far.  After an
        interior solve: the boundary queries; a first step: every query (levels 0..``level`` are exact with this halo); a
        straggler round: only the queries left unfinished, over own + widened halo tree.  Every other row stays."""
        rows_of = lambda res: {kk: v for kk, v in res.items() if kk != "info"}  # noqa: E731
        if interior is not None:
            res = self.engine.solve(k, float(r0), out=rows_of(interior["res"]), phase=2, **solve_kw)
            res["info"] = self._merge_infos(interior["res"]["info"], res["info"], 0)
        elif st.res is None:
            res = self.engine.solve(k, float(r0), **solve_kw)
        else:
            before = st.res["info"]
            res = self.engine.solve(k, float(r0), out=rows_of(st.res), phase=3, **solve_kw)
            res["info"] = self._merge_infos(before, res["info"], int(before["unfinished"]) * level)
        st.res = res

    def _anyone_left(self, info):
        """ONE all-reduce per step: (no rank has unfinished queries -- a maximum says so as well as a sum --, most rounds)"""
        left = torch.tensor([int(info["unfinished"]), int(info["rounds"])], dtype=torch.int64, device=self.device)
        unfinished, rounds = self.comm.all_reduce(left, dist.ReduceOp.MAX).tolist()
        return int(unfinished) == 0, int(rounds)

    def solve(self, k, start_radius, max_rounds=64, want_fb=False):
        r0 = np.float32(start_radius)
        level = self._first_halo_level(k, r0)
        clock = _PhaseClock(("select", "exchange", "halo_build", "solve", "reduce"), self.device, self.profile)
        st = _SolveState(self.comm.world)
        while True:
            tag = ("halo", level, st.res is None)
            halo_radius = self._halo_radius(r0, level)
            solve_kw = dict(kernel=self.kernel, max_rounds=level + 1, want_fb=want_fb, want_levels=True, allow_unfinished=True)
            clock.restart()
            blocks, selection = self._select(st, tag, halo_radius)
            clock.lap("select")
            with self._interior_solve(st, k, r0, want_fb, solve_kw) as interior:
                self._exchange(st, tag, blocks, selection, halo_radius, clock)
            if interior is not None:
                clock.ms["interior_solve_overlapped"] = interior["ms"]  # (a first step's: once per solve)
                clock.restart()
            self._engine_step(st, k, r0, level, interior, solve_kw)
            clock.lap("solve")
            done, rounds_all = self._anyone_left(st.res["info"])
            clock.lap("reduce")
            if done:
                break
            if level + 1 >= max_rounds:
                raise _lib.TknnError(-4, "max_rounds reached with unfinished queries")
            level += 1  # stragglers need the next radius level: widen the halo by its shell and solve them again
        # (halo_points_by_exchange: the first exchange's halo, then the shells of the straggler rounds)
        info = dict(st.res["info"], rounds=rounds_all, halo_exchanges=len(st.round_halo), halo_points=len(st.halo),
                    halo_points_by_exchange=st.round_halo, halo_levels=level, overlapped=st.overlapped, halo_select_one_pass=st.one_pass)
        if self.profile:
            info["phase_ms"] = clock.ms
        self.last = st.res
        self.last["info"] = info
        return info

    # ---- RT-DBSCAN over the tiles (last row) -----------------------------------
    def dbscan(self, eps, min_pts, _reuse_setup=False):
        """DBSCAN of the whole set with the single-GPU spec (oracle/dbscan_oracle.c): returns
        dict(labels (m,) int32, core (m,) bool) for the points this rank owns (``self.ids`` order) and
        info(clusters, rounds, halo_points).  Clusters are numbered by ascending smallest core id, so
        the labels equal a single-process run over the union.

        Each rank clusters its tile plus a halo of radius 2 eps: core flags are then exact for its own
        points and for every foreign point that can be their neighbour, and every edge of the
        neighbour graph is seen by a rank owning one of its ends.  Components are merged by label
        propagation: label = smallest core id known for the component; a round takes the minimum
        over each local component, sends the labels of halo copies back to their owners (minimum) and
        the owners' labels out to the copies again, until nothing changes anywhere."""
        dev, eps32, m = self.device, float(np.float32(eps)), len(self.points)
        clock = _PhaseClock(("setup", "cluster", "propagate", "number", "assign"), dev, self.profile)
        halo, counts_in, sent_local, ids = self._db_setup(eps32, reuse=_reuse_setup)
        clock.lap("setup")
        local = self.db_engine.dbscan(eps32, min_pts)
        clock.lap("cluster")
        core = local["core"].to(dev).bool()
        # Label propagation works on CLUSTERS, not points (round 4; the per-point form spent 160 ms of a 174 ms step in
        # scatter-reduces of ten million values onto 83 addresses): lab_comp[c] = the smallest global core id known for local
        # cluster c.  Per point there is one step before the rounds (the clusters' own minima: tknnSegmentMin) and one gather
        # after them; a round moves the values of the halo rows and touches the clusters they belong to.
        seg = torch.where(core, local["labels"].to(dev).int(), torch.full((len(ids),), -1, dtype=torch.int32, device=dev))  # cluster of a core point, else -1
        ncomp = int((local.get("info") or {}).get("clusters", -1))
        if ncomp < 0:  # (an engine that does not say)
            ncomp = int(seg.max().item()) + 1 if len(seg) else 0
        ncomp = max(ncomp, 0)
        lab_comp = torch.full((max(ncomp, 1),), _BIG, dtype=torch.int64, device=dev)
        self._seg_min(seg, ids.long(), lab_comp)
        rounds = self._propagate_labels(lab_comp, seg, m, counts_in, sent_local)
        clock.lap("propagate")
        clusters, core_label = self._number_clusters(lab_comp, seg, ids, m)
        clock.lap("number")
        labels = self.db_engine.dbscan_assign(eps32, core_label)
        clock.lap("assign")
        info = {"clusters": clusters, "rounds": rounds, "label_rounds": rounds, "halo_points": int(len(halo)), "halo_exchanges": 1}
        # the tile's own clustering as its engine reports it (device times of the three traversal kernels, work counters)
        eng_info = dict(local.get("info") or {})
        eng_info["n_clustered"] = int(len(ids))
        info["engine"] = eng_info
        if self.profile:
            info["phase_ms"] = clock.ms
        return {"labels": labels[:m].to(dev), "core": core[:m], "info": info}

    def _propagate_labels(self, lab_comp, seg, m, counts_in, sent_local):
        """Label propagation between the ranks, in place on ``lab_comp`` (per local cluster, the smallest global core id
        known): a round sends the labels of the halo copies back to their owners (minimum) and the owners' labels out to
        the copies again, until a round changes nothing on any rank.  Returns the number of rounds."""
        comm, dev = self.comm, self.device
        seg_halo = seg[m:]
        seg_sent = [seg[:m][sent_local[p]] if len(sent_local[p]) else seg[:0] for p in range(comm.world)]
        offs = np.concatenate([[0], np.cumsum(counts_in)])
        big_row = torch.full((1,), _BIG, dtype=torch.int64, device=dev)

        def of_clusters(which):  # the clusters' labels for a list of rows (a row that is not core: nothing to say)
            return torch.where(which >= 0, lab_comp[which.clamp(min=0).long()], big_row).reshape(-1, 1).contiguous()

        def answer(blocks, expect):  # (both directions answer rows that travelled before: every count is known at both ends)
            expect = [int(len(blocks[p])) if p == comm.rank else int(c) for p, c in enumerate(expect)]
            return comm.exchange_rows(blocks, 1, torch.int64, dev, counts_in=expect)

        rounds = 0
        while True:
            rounds += 1
            before = lab_comp.clone()
            # copies -> owners (minimum)
            back = [of_clusters(seg_halo[int(offs[s_]): int(offs[s_ + 1])]) for s_ in range(comm.world)]
            for p, vals in enumerate(answer(back, [len(s_) for s_ in sent_local])):
                if p != comm.rank and len(vals):
                    self._seg_min(seg_sent[p], vals.flatten(), lab_comp)
            # owners -> copies
            new = answer([of_clusters(seg_sent[p]) for p in range(comm.world)], counts_in)
            new[comm.rank] = new[comm.rank][:0]
            if len(seg_halo):
                self._seg_min(seg_halo, torch.cat(new, dim=0).flatten(), lab_comp)
            changed = torch.tensor([int(bool((lab_comp != before).any()))], dtype=torch.int64, device=dev)
            comm.all_reduce(changed, dist.ReduceOp.MAX)
            if int(changed.item()) == 0:
                return rounds

    def _number_clusters(self, lab_comp, seg, ids, m):
        """Global cluster numbers: ascending smallest core id over ALL ranks (a rank contributes the clusters that have a
        core point of its OWN).  Returns (number of clusters, per row of ``seg`` the number of its cluster or -1)."""
        comm, dev = self.comm, self.device
        own_min = torch.full_like(lab_comp, _BIG)
        self._seg_min(seg[:m], ids[:m].long(), own_min)
        mine = torch.unique(lab_comp[own_min != _BIG])
        width = torch.tensor([len(mine)], dtype=torch.int64, device=dev)
        comm.all_reduce(width, dist.ReduceOp.MAX)
        padded = torch.full((max(int(width.item()), 1),), _BIG, dtype=torch.int64, device=dev)
        padded[: len(mine)] = mine
        everyone = torch.unique(comm.all_gather(padded).flatten())
        everyone = everyone[everyone != _BIG]
        number_comp = torch.searchsorted(everyone, lab_comp.clamp(max=int(everyone[-1].item()) if len(everyone) else 0)).int()
        core_label = torch.where(seg >= 0, number_comp[seg.clamp(min=0).long()], torch.full_like(seg, -1))
        return int(len(everyone)), core_label

    def _seg_min(self, seg, val, out):
        """out[seg[i]] = min(out[seg[i]], val[i]) for seg[i] >= 0: the engine's kernel (tknnSegmentMin) if it has one, else torch"""
        if len(seg) == 0:
            return out
        if hasattr(self.db_engine, "segment_min"):
            return self.db_engine.segment_min(seg.int(), val, out)
        keep = seg >= 0
        if bool(keep.any()):
            out.scatter_reduce_(0, seg[keep].long(), val[keep], "amin")
        return out

    def _db_setup(self, eps32, reuse=False):
        """The engine over my tile plus a halo of radius 2 eps (see dbscan).  ``reuse``: the auto-eps loop's last growth
        round and the clustering that follows it use one exchange and one tree; every other call does its own."""
        if reuse and self._db_cache is not None and self._db_cache[0] == eps32:
            return self._db_cache[1]
        comm, dev = self.comm, self.device
        blocks = self._halo_blocks(2.0 * eps32)
        got = comm.exchange_rows(blocks, 4, torch.float32, dev)
        got[comm.rank] = got[comm.rank][:0]
        counts_in = [len(g) for g in got]
        halo = torch.cat(got, dim=0)
        # the rows I sent, as positions in my own arrays (values travel in the same order later)
        id_sorted, id_perm = torch.sort(self.ids.long())
        sent_local = [id_perm[torch.searchsorted(id_sorted, b[:, 3].contiguous().view(torch.int32).long())]
                      if len(b) else torch.zeros(0, dtype=torch.long, device=dev) for b in blocks]
        pts = torch.cat([self.points, halo[:, :3]], dim=0).contiguous()
        ids = torch.cat([self.ids, halo[:, 3].contiguous().view(torch.int32)], dim=0).contiguous()
        if self.db_engine is None:
            self.db_engine = self._engine_factory(dev)
        self.db_engine.build(pts, ids)
        self._db_cache = (eps32, (halo, counts_in, sent_local, ids))
        return self._db_cache[1]

    def dbscan_auto(self, eps0, min_pts, max_noise=0.05, max_rounds=32):
        """RT-DBSCAN with an auto-grown eps over the tiles (spec: oracle/dbscan_oracle.c, dbref_dbscan_auto): rounds of the
        eps doubling (fp32, hostCode.cpp:321) until at most floor(max_noise * n_total) points of the WHOLE set are noise.
        A growth round exchanges the 2-eps halo, builds the tile's tree and counts its own noise points
        (tknnDbscanNoise) -- one 8-byte all-reduce per round; clusters are built once, at the final eps."""
        comm, dev = self.comm, self.device
        bound = int(np.floor(float(max_noise) * self.n_total))
        eps = np.float32(eps0)
        m = len(self.points)
        for t in range(int(max_rounds)):
            # a growth round only counts: core flags are exact for my own points inside the 2-eps halo, and a point of
            # mine is noise iff it is not core and has no core point within eps -- no clusters, no label exchange
            self._db_setup(float(eps))
            flags = self.db_engine.dbscan_noise(float(eps), min_pts)["noise"]
            noise = torch.tensor([int(flags[:m].sum().item())], dtype=torch.int64, device=dev)
            comm.all_reduce(noise, dist.ReduceOp.SUM)
            if int(noise.item()) <= bound:
                r = self.dbscan(float(eps), min_pts, _reuse_setup=True)  # (same eps: the round's halo and tree)
                # "rounds" = growth rounds, as in tknnDbscanAutoInfo; the label propagation's rounds stay in "label_rounds"
                r["info"].update({"rounds": t + 1, "eps_rounds": t + 1, "eps": float(eps), "noise": int(noise.item())})
                return r
            eps = np.float32(eps * np.float32(2))
        raise _lib.TknnError(-4, "max_rounds doublings of eps did not bring the noise under the bound")

    def gather_rows(self):
        """(global_ids, idx, dist, intersections) of every rank concatenated on every rank (tests)."""
        comm, dev = self.comm, self.device
        k = self.last["idx"].shape[1]
        rows = torch.cat([self.ids.view(-1, 1).to(torch.float64), self.last["idx"].to(torch.float64),
                          self.last["dist"].to(torch.float64),
                          self.last["intersections"].view(-1, 1).to(torch.float64)], dim=1)
        blocks = [rows for _ in range(comm.world)]
        got = torch.cat(comm.exchange_rows(blocks, rows.shape[1], torch.float64, dev), dim=0).cpu().numpy()
        order = np.argsort(got[:, 0])
        got = got[order]
        return (got[:, 0].astype(np.int64), got[:, 1:1 + k].astype(np.int32),
                got[:, 1 + k:1 + 2 * k].astype(np.float32), got[:, 1 + 2 * k].astype(np.int64))
