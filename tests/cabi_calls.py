"""Every tknn* call of include/owlknn.h that takes an engine, with plausible arguments: what the boundary tests
(test_cabi.py without a GPU, test_cabi_refusals_gpu.py with one) start from before they put ONE fault into a call.

A call's arguments are listed by name in the C order, without the engine in front and without info and stream behind.
``DEV`` stands for "an address in device memory", ``HOST`` for one in host memory, ``COUNT`` for a host int64 the call may
write; the caller says what those addresses are.  A ``(Structure, fields)`` pair is an options record passed by address."""
import ctypes

from owlraytracing_amd import _lib

OK, E_ARG, E_HIP, E_STATE, E_ROUNDS, E_UNSUPPORTED = 0, -1, -2, -3, -4, -5
DEV, HOST, COUNT = "device address", "host address", "host int64"
TOO_MANY = 0x7fffffff  # the first count the library refuses (counts are < 2^31 - 1)

CALLS = {
    "tknnBuild": (dict(d_xyz=DEV, n=10), _lib.BuildInfo),
    "tknnBuildIds": (dict(d_xyz=DEV, d_ids=None, n=10), _lib.BuildInfo),
    "tknnSetHalo": (dict(d_xyz=DEV, d_ids=DEV, m=4), None),
    "tknnHaloSelect": (dict(d_boxes=DEV, d_box_peer=DEV, nboxes=1, npeers=1, d_counts=DEV, d_offsets=None, d_rows=None), None),
    "tknnHaloSelectFixed": (dict(d_boxes=DEV, d_box_peer=DEV, nboxes=1, npeers=1, d_caps=DEV, d_offsets=DEV, d_rows=DEV, d_counts=DEV), None),
    "tknnSolve": (dict(k=3, start_radius=0.1, kernel=0, max_rounds=0, d_idx=DEV, d_dist=DEV, d_intersections=DEV, d_fb=None), _lib.SolveInfo),
    "tknnSolveEx": (dict(options=(_lib.SolveOptions, dict(k=3, start_radius=0.1, d_idx=DEV, d_dist=DEV, d_intersections=DEV))), _lib.SolveInfo),
    "tknnRepairExact": (dict(k=3, start_radius=0.1, d_levels=DEV, d_idx=DEV, d_dist=DEV, repaired=COUNT), None),
    "tknnQuery": (dict(options=(_lib.QueryOptions, dict(d_queries=DEV, m=4, k=3, start_radius=0.1, d_idx=DEV, d_dist=DEV, d_intersections=DEV))),
                  _lib.SolveInfo),
    "tknnDbscan": (dict(eps=0.1, min_pts=3, d_labels=DEV, d_core=DEV, d_counts=None), _lib.DbscanInfo),
    "tknnDbscanAssign": (dict(eps=0.1, d_core_label=DEV, d_labels=DEV), _lib.DbscanInfo),
    "tknnDbscanQuery": (dict(options=(_lib.DbscanQueryOptions, dict(d_queries=DEV, m=4, eps=0.1, d_core_label=DEV, d_labels=DEV))), _lib.DbscanInfo),
    "tknnRadiusQuery": (dict(options=(_lib.RadiusOptions, dict(d_queries=DEV, m=4, radius=0.1, sort=1, d_offsets=DEV))), _lib.RadiusInfo),
    "tknnRadiusKnn": (dict(options=(_lib.RadiusKnnOptions, dict(d_queries=DEV, m=4, k=3, radius=0.1, d_idx=DEV, d_dist=DEV, d_counts=DEV))),
                      _lib.RadiusKnnInfo),
    "tknnDbscanAuto": (dict(eps0=0.1, min_pts=3, max_noise=0.05, max_rounds=8, d_labels=DEV, d_core=DEV), _lib.DbscanAutoInfo),
    "tknnDbscanNoise": (dict(eps=0.1, min_pts=3, d_noise=DEV, noise_count=COUNT), None),
    "tknnSegmentMin": (dict(d_segment=DEV, d_value=DEV, n=4, d_out=DEV), None),
    "tknnExportTree": (dict(nodes=HOST, rope_node=HOST, rope_leaf=HOST, prim_id=HOST), None),
    "tknnExportTreeTables": (dict(split_owner=HOST, block_paths=HOST), None),
    "tknnExportTreeEx": (dict(x=(_lib.TreeExport, dict(which=0, wide_boxes=HOST, wide_capacity=8))), None),
}

# the name a call's messages start with: the thin forms speak as the call they forward to, the two forms of the halo
# selection share the engine's function and what it says
SPEAKS_AS = {"tknnBuildIds": "tknnBuild", "tknnSolveEx": "tknnSolve", "tknnHaloSelectFixed": "tknnHaloSelect"}

INFO_FILL = 0xA5  # an info record is handed over filled with this byte: a refused call leaves it so, an accepted one zeroes it


def call(lib, fn, engine, dev, host, **faults):
    """Calls ``fn`` on ``engine`` with CALLS' arguments, ``faults`` in place of those they name (an argument, or a field of
    the call's options record; the record's own name with None passes NULL for it).  Returns (code, message, info bytes or
    None, the options record or None)."""
    spec, info_cls = CALLS[fn]
    left = dict(faults)
    where = {DEV: dev, HOST: host}
    args, record = [], None
    for name, v in spec.items():
        if isinstance(v, tuple):
            cls, fields = v
            if name in left:
                assert left.pop(name) is None
                args.append(None)
                continue
            record = cls()
            fields = dict(fields)
            for field, _ in cls._fields_:
                if field in left:
                    fields[field] = left.pop(field)
            for field, f in fields.items():
                setattr(record, field, where.get(f, f) if isinstance(f, str) else f)
            args.append(ctypes.byref(record))
            continue
        v = left.pop(name, v)
        if isinstance(v, str) and v == COUNT:
            args.append(ctypes.byref(ctypes.c_int64(-7)))
        else:
            args.append(where.get(v, v) if isinstance(v, str) else v)
    assert not left, "%s has no argument %s" % (fn, sorted(left))
    info = None
    if info_cls is not None:
        info = info_cls()
        ctypes.memset(ctypes.byref(info), INFO_FILL, ctypes.sizeof(info))
        args.append(ctypes.byref(info))
    rc = getattr(lib, fn)(engine, *args, None)
    message = (lib.tknnLastError() or b"").decode() if rc != OK else ""
    return rc, message, None if info is None else bytes(info), record
