#!/usr/bin/env python3
"""Command line of the reference sample, served by the fused engine:

    tools/trueknn_cli.py <points.csv> <n> <dim> <start_radius|auto> <k> <timefile> [--out rows.npz]
                         [--queries <queries.csv> [--exact]]

Arguments as samples/s01-trueknn/hostCode.cpp:66-73; prints the same "Build time" / "True KNN time"
/ "Total time" lines (hostCode.cpp:211,344-347) and appends the total to <timefile> (:349-356).
`auto` takes the start radius from owlraytracing_amd.radius.sample_start_radius.
With --queries the rows are those of the points in that file (same format, every line of it) against the set, not of
the set itself (TrueKNN.query), and they are printed: one line "j: idx ... | dist ..." per query; --exact asks for exact kNN.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file")
    ap.add_argument("n", type=int)
    ap.add_argument("dim", type=int)
    ap.add_argument("start_radius")
    ap.add_argument("k", type=int)
    ap.add_argument("timefile")
    ap.add_argument("--out", default=None, help="write idx/dist/intersections/levels as .npz (tools/compare_reference_dump.py --rows reads it)")
    ap.add_argument("--kernel", type=int, default=0)
    ap.add_argument("--queries", default=None, help="CSV of query points (same reader as the points): answer for them instead of the set itself")
    ap.add_argument("--exact", action="store_true", help="with --queries: exact kNN rows in (dist, index) order")
    a = ap.parse_args()

    from owlraytracing_amd import datasets
    from owlraytracing_amd.radius import sample_start_radius
    from owlraytracing_amd.trueknn import TrueKNN

    pts = datasets.pad_to_3d(datasets.read_csv_points(a.file, a.n, a.dim))
    print("#owl.sample(main):  num spheres: %d" % len(pts))
    r0 = sample_start_radius(pts) if a.start_radius == "auto" else float(a.start_radius)
    eng = TrueKNN()
    b = eng.build(pts)
    print("Build time: %g seconds." % (b["build_ms"] / 1e3))
    if a.exact and not a.queries:
        ap.error("--exact goes with --queries")
    if a.queries:
        with open(a.queries) as fh:
            m = sum(1 for line in fh if line.strip())
        qs = datasets.pad_to_3d(datasets.read_csv_points(a.queries, m, a.dim))
        print("#owl.sample(main):  num queries: %d" % len(qs))
        r = eng.query(qs, a.k, r0, exact=a.exact, want_levels=True)
        idx, dist = r["idx"].cpu().numpy(), r["dist"].cpu().numpy()
        for j in range(len(qs)):
            print("%d: %s | %s" % (j, " ".join(str(int(v)) for v in idx[j]), " ".join(repr(float(v)) for v in dist[j])))
    else:
        r = eng.solve(a.k, r0, kernel=a.kernel, want_levels=True)
    info = r["info"]
    print("Rounds: %d  start radius %g  final radius %g" % (info["rounds"], r0, info["final_radius"]))
    print("True KNN time: %g seconds." % (info["solve_ms"] / 1e3))
    tot = (b["build_ms"] + info["solve_ms"]) / 1e3
    print("Total time: %g" % tot)
    with open(a.timefile, "a") as fh:
        fh.write("%g\n" % tot)
    if a.out:
        np.savez(a.out, idx=r["idx"].cpu().numpy(), dist=r["dist"].cpu().numpy(),
                 intersections=r["intersections"].cpu().numpy(), levels=r["levels"].cpu().numpy())
    eng.close()


if __name__ == "__main__":
    main()
