#!/usr/bin/env python3
"""Generate tests/golden/rknn_counters.json -- the work counters of the four radius-bounded kNN calls (tknnRadiusKnn, tknnKnn,
tknnPeriodicKnn, tknnBatchKnn) on one small set, as the build that runs this script reports them.

The rows of these calls are pinned bit for bit by their own tests.  This fixture pins the WORK behind the rows: a change of the
walk, seed or lane kernels that is meant to leave them alone must report the same totals, node tests and point tests, not only
the same rows.  The counters are reproducible from run to run: the walk's cursor hands out fixed groups of four sorted positions,
and the wave-wide merge triggers depend only on the group.

20 000 uniform points; 1 000 external queries and the set's own points; k = 10 and 17 (one and two list registers per lane);
tknnRadiusKnn at a radius that leaves full and short rows, tknnKnn, tknnPeriodicKnn and tknnBatchKnn (7 batches) without and with
that radius; and one case per call under its TKNN_*_FORCE_FALLBACK=1, where the one-query-per-lane kernel does all the work.
Per case the info counters of COUNTERS that the call's record has.

Run on a GPU, from the repo root, on the build whose work is to be the reference:  python tests/golden/make_rknn_counters.py
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rknn_counters.json")
COUNTERS = ("total", "full_rows", "node_tests", "point_tests", "seed_point_tests", "tightened_rows", "lane_rows")
N, M, BATCHES, RADIUS = 20000, 1000, 7, 0.05  # some 10 points within RADIUS of a point
FALLBACK = {"radius_knn": "TKNN_RADIUS_KNN_FORCE_FALLBACK", "knn": "TKNN_KNN_FORCE_FALLBACK",
            "periodic_knn": "TKNN_PERIODIC_KNN_FORCE_FALLBACK", "batch_knn": "TKNN_BATCH_KNN_FORCE_FALLBACK"}


def inputs():
    from owlraytracing_amd import datasets

    rng = np.random.default_rng(4711)
    P = datasets.uniform3d(N, seed=0)
    Q = rng.random((M, 3), dtype=np.float32)
    return P, Q, rng.integers(0, BATCHES, N).astype(np.int32), rng.integers(0, BATCHES, M).astype(np.int32)


def cases():
    """(name, call, own, k, radius, forced): `call` names the engine's method, `own` the set's own points as the queries."""
    for own in (False, True):
        for k in (10, 17):
            for call, radius in (("radius_knn", RADIUS), ("knn", None), ("periodic_knn", None), ("periodic_knn", RADIUS),
                                 ("batch_knn", None), ("batch_knn", RADIUS)):
                yield "%s %s k=%d%s" % (call, "own" if own else "ext", k, "" if radius is None or call == "radius_knn" else " r"), call, own, k, radius, False
    yield "radius_knn ext k=17 lane", "radius_knn", False, 17, RADIUS, True
    yield "knn own k=10 lane", "knn", True, 10, None, True
    yield "periodic_knn ext k=10 r lane", "periodic_knn", False, 10, RADIUS, True
    yield "batch_knn own k=17 lane", "batch_knn", True, 17, None, True


class Engines:
    """The plain tree and the batched one over the same points, and every case's call."""

    def __init__(self):
        from owlraytracing_amd.trueknn import TrueKNN

        self.P, self.Q, self.batch, self.query_batch = inputs()
        self.plain, self.batched = TrueKNN(device=0), TrueKNN(device=0)
        self.plain.build(self.P)
        self.batched.build(self.P, batch=self.batch, num_batches=BATCHES)

    def close(self):
        self.plain.close()
        self.batched.close()

    def run(self, call, own, k, radius, forced):
        """The info record of one case."""
        rad = {} if radius is None else {"radius": radius}
        if forced:
            os.environ[FALLBACK[call]] = "1"
        try:
            if call == "radius_knn":
                res = self.plain.radius_knn(self.P if own else self.Q, k, radius=radius, skip_ids=np.arange(N, dtype=np.int32) if own else None)
            elif call == "knn":
                res = self.plain.knn(None if own else self.Q, k)
            elif call == "periodic_knn":
                res = self.plain.periodic_knn(None if own else self.Q, k, lo=0.0, period=1.0, **rad)
            else:
                res = self.batched.batch_knn(None if own else self.Q, k, batch=None if own else self.query_batch, **rad)
        finally:
            if forced:
                del os.environ[FALLBACK[call]]
        return res["info"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    eng = Engines()
    rec = {}
    for name, call, own, k, radius, forced in cases():
        info = eng.run(call, own, k, radius, forced)
        m = N if own else M
        assert info["lane_rows"] == (m if forced else 0), (name, info)
        if call == "radius_knn":
            assert 0 < info["full_rows"] < m, (name, info)  # full and short rows
        rec[name] = {c: int(info[c]) for c in COUNTERS if c in info}
        print("%-32s %s" % (name, rec[name]))
    eng.close()
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
