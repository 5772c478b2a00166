#!/usr/bin/env python3
"""Generate tests/golden/queries/*.npz -- small fixtures for queries that are not in the set (tknnQuery).

Every row comes from the append-one-query identity: row j = oracle.trueknn_rows(concat(P, q_j), k, r, query_ids=[n]),
the row the replay of the reference's loop gives q_j in P + {q_j}; level = its rounds - 1, intersections = its counter
minus the query's own box once per traced level.  Each file holds
  points (n,3) f32 | queries (m,3) f32 | k | start_radius | idx (m,k) i32 | dist (m,k) f32 | intersections (m,) i64 | levels (m,) i32

Run from the repo root:  python tests/golden/queries/make_query_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
import query_spec as qs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def identity_rows(P, Q, k, r0):
    n = len(P)
    idx, dist = np.empty((len(Q), k), np.int32), np.empty((len(Q), k), np.float32)
    isect, levels = np.empty(len(Q), np.int64), np.empty(len(Q), np.int32)
    for j in range(len(Q)):
        o = oracle.trueknn_rows(np.concatenate([P, Q[j:j + 1]]), k, r0, np.array([n], np.int32))
        levels[j] = o["rounds"] - 1
        idx[j], dist[j] = o["idx"][0], o["dist"][0]
        isect[j] = o["intersections"][0] - o["rounds"]
    return idx, dist, isect, levels


def cases():
    P, Q, r0 = qs.make_set("uniform")
    yield "uniform_n20000_m150_k10", P, np.concatenate([Q[:100], Q[-50:]]), 10, r0
    P, Q, r0 = qs.make_set("lattice")
    yield "lattice_n1398_m300_k10", P, Q[::2], 10, r0
    P, Q, r0 = qs.make_set("duplicates")
    yield "duplicates_n4000_m200_k5", P, np.concatenate([Q[:100], Q[-100:]]), 5, r0


if __name__ == "__main__":
    for name, P, Q, k, r0 in cases():
        idx, dist, isect, levels = identity_rows(P, Q, k, r0)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, points=P, queries=Q, k=k, start_radius=np.float32(r0), idx=idx, dist=dist, intersections=isect, levels=levels)
        print("%s: %d bytes" % (name, os.path.getsize(path)))
