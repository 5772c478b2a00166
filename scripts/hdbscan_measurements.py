#!/usr/bin/env python3
"""Times of tknnHdbscan and of the steps behind the spanning tree (tknnHdbscanLabels: dendrogram, condensed tree, selection,
labels) on one MI355X, written to profiles/hdbscan_measurements.json (--out; sets measured in
several runs are joined by hand: one "cases" list).

Sets: 1 M and 10 M uniform points, 10 M points of a 64-component mixture; min_samples 1 and 5, min_cluster_size 5 and 100.  Per
case 1 warm-up and --reps timed calls: the time between two HIP events around the call and the phase times the call reports
(knn, emst, linkage, condense, select, label), the contraction rounds, host_edges (expected 0), clusters and noise.  Per
(set, min_samples) once: the records absorbed in each round -- tknnLinkage repeated with max_rounds = 1, 2, ..., whose info says
how many records the rounds absorbed before the host took the rest; the differences are the rounds'.
Two yardsticks, neither the code under test:
  * tknnEmst on the same engine with the same core distances, timed the same way in the same run: `post_tree_over_emst` =
    tknnHdbscanLabels / tknnEmst, medians of the events;
  * at n <= --host-recipe-max (1 M): the host recipe -- the records copied to the host, sklearn's make_single_linkage +
    tree_to_labels (eom, no single cluster) on the CPU, wall clock: one untimed run first, then one timed run per
    min_cluster_size.  Where sklearn's private modules are missing the field says so.  `same_partition_as_sklearn` compares the
    two labellings up to renumbering (they may differ: sklearn gives ties to the children and takes w = 0 as an infinite lambda).
Checks before anything is timed: the call's records are tknnEmst's, bit for bit; labels from the records alone equal the call's;
every label's cluster has at least min_cluster_size points; noise + labelled = n.

    python scripts/hdbscan_measurements.py [--sets uniform:1000000,uniform:10000000,mixture:10000000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from emst_measurements import timed  # noqa: E402
from radius_measurements import stats  # noqa: E402

MIN_SAMPLES = (1, 5)
MIN_CLUSTER_SIZES = (5, 100)
PHASES = ("solve_ms", "knn_ms", "emst_ms", "linkage_ms", "condense_ms", "select_ms", "label_ms")


def absorbed_per_round(eng, u, v, n, rounds):
    out, before = [], 0
    for r in range(1, rounds + 1):
        info = eng.linkage(u, v, n=n, max_rounds=r)["info"]
        assert info["rounds"] == r and info["absorbed"] + info["host_edges"] == len(u), info
        out.append(int(info["absorbed"] - before))
        before = info["absorbed"]
    return out


def sklearn_recipe(u, v, w, min_cluster_size):
    """(labels, seconds) of the host recipe on records already on the host, or (None, why)."""
    try:
        from sklearn.cluster._hdbscan import _linkage, _tree
    except Exception as e:  # the modules are private: another sklearn may keep them elsewhere
        return None, "sklearn's tree code not importable: %s" % e
    t0 = time.perf_counter()
    mst = np.zeros(len(u), dtype=_linkage.MST_edge_dtype)
    mst["current_node"], mst["next_node"], mst["distance"] = u, v, w
    labels = _tree.tree_to_labels(_linkage.make_single_linkage(mst), min_cluster_size, "eom", False, 0.0, None)[0]
    return labels, time.perf_counter() - t0


def same_partition(a, b):
    key = a.astype(np.int64) * (int(b.max()) + 2) + b
    pairs = len(np.unique(key))
    return bool(pairs == len(np.unique(a)) == len(np.unique(b)) and np.array_equal(a < 0, b < 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="uniform:1000000,uniform:10000000,mixture:10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-recipe-max", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdbscan_measurements.json"))
    a = ap.parse_args()

    import torch

    from owlraytracing_amd import _lib, datasets
    from owlraytracing_amd.trueknn import TrueKNN

    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmups": 1, "checks": "ok", "source_fingerprint": _lib.source_fingerprint(),
           "cases": []}
    for spec in a.sets.split(","):
        kind, n = spec.split(":")
        n = int(n)
        P = datasets.uniform3d(n, seed=0) if kind == "uniform" else datasets.gaussian_mixture3d(n, components=64, sigma=0.02, seed=1)
        P = np.ascontiguousarray(P, np.float32)
        eng = TrueKNN(device=0)
        eng.build(P)
        for min_samples in MIN_SAMPLES:
            core = None if min_samples == 1 else eng.knn(k=min_samples - 1)["dist"][:, -1].contiguous()
            tree = eng.emst(core_dist=core)  # warm-up
            emst_wall, emst_infos = timed(lambda: eng.emst(core_dist=core), a.reps)
            u, v, w = tree["u"], tree["v"], tree["w"]
            rounds_absorbed = None
            host = None
            for mcs in MIN_CLUSTER_SIZES:
                got = eng.hdbscan(mcs, min_samples, want_tree=True)  # warm-up: the result is checked
                alone = eng.hdbscan_labels(u, v, w, n, mcs)  # warm-up
                lab = got["labels"]
                counts = torch.bincount(lab[lab >= 0].to(torch.int64), minlength=1)
                ok = (all(torch.equal(got[f].view(torch.int32), tree[f].view(torch.int32)) for f in ("u", "v", "w")) and torch.equal(lab, alone["labels"])
                      and int((lab < 0).sum()) == got["info"]["noise"] and int(lab.max()) + 1 == got["info"]["clusters"]
                      and (got["info"]["clusters"] == 0 or int(counts.min()) >= mcs))
                print("%s n=%d min_samples=%d min_cluster_size=%d: checks %s" % (kind, n, min_samples, mcs, "ok" if ok else "MISMATCH"), flush=True)
                if not ok:
                    sys.exit(1)
                if rounds_absorbed is None:
                    rounds_absorbed = absorbed_per_round(eng, u, v, n, alone["info"]["rounds"])
                labels_host = lab.cpu().numpy()
                del got, alone
                wall, infos = timed(lambda: eng.hdbscan(mcs, min_samples), a.reps)
                post_wall, post_infos = timed(lambda: eng.hdbscan_labels(u, v, w, n, mcs), a.reps)
                last = infos[-1]
                case = {"set": kind, "n": n, "min_samples": min_samples, "min_cluster_size": mcs, "events_ms": stats(wall),
                        "device_ms": {key: stats([i[key] for i in infos]) for key in PHASES},
                        "post_tree_events_ms": stats(post_wall),
                        "post_tree_device_ms": {key: stats([i[key] for i in post_infos]) for key in PHASES if key not in ("knn_ms", "emst_ms")},
                        "emst_events_ms": stats(emst_wall), "emst_device_ms": stats([i["solve_ms"] for i in emst_infos]),
                        "rounds": last["rounds"], "absorbed_per_round": rounds_absorbed, "host_edges": last["host_edges"], "edges": last["edges"],
                        "excluded": last["excluded"], "clusters": last["clusters"], "noise": last["noise"], "condensed_clusters": last["condensed_clusters"]}
                case["post_tree_over_emst"] = case["post_tree_events_ms"]["median"] / case["emst_events_ms"]["median"]
                if n <= a.host_recipe_max:
                    t0 = time.perf_counter()
                    hu, hv, hw = u.cpu().numpy(), v.cpu().numpy(), w.cpu().numpy()
                    copy_s = time.perf_counter() - t0
                    if host is None:
                        host = sklearn_recipe(hu, hv, hw, MIN_CLUSTER_SIZES[-1])  # untimed: first call
                    sk_labels, sk = sklearn_recipe(hu, hv, hw, mcs)
                    if sk_labels is None:
                        case["host_recipe"] = sk
                    else:
                        case["host_recipe"] = {"copy_ms": copy_s * 1e3, "sklearn_ms": sk * 1e3, "same_partition_as_sklearn": same_partition(labels_host, sk_labels),
                                               "sklearn_clusters": int(sk_labels.max()) + 1, "sklearn_noise": int((sk_labels < 0).sum())}
                        case["host_recipe_over_post_tree"] = (copy_s + sk) * 1e3 / case["post_tree_events_ms"]["median"]
                print("  hdbscan %.2f ms: knn %.2f emst %.2f linkage %.2f condense %.2f select %.2f label %.2f; %d rounds %s, host_edges %d; %d clusters, %d noise"
                      % (case["events_ms"]["median"], last["knn_ms"], last["emst_ms"], last["linkage_ms"], last["condense_ms"], last["select_ms"], last["label_ms"],
                         last["rounds"], rounds_absorbed, last["host_edges"], last["clusters"], last["noise"]), flush=True)
                print("  post-tree %.2f ms = %.3f x emst (%.2f ms)%s" % (case["post_tree_events_ms"]["median"], case["post_tree_over_emst"], case["emst_events_ms"]["median"],
                                                                        "; host recipe %s" % (case.get("host_recipe"),) if "host_recipe" in case else ""), flush=True)
                rec["cases"].append(case)
                os.makedirs(os.path.dirname(a.out), exist_ok=True)
                with open(a.out, "w") as fh:  # after every case: a run cut short keeps what it measured
                    json.dump(rec, fh, indent=1)
            del core, tree, u, v, w
            torch.cuda.empty_cache()
        eng.close()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
