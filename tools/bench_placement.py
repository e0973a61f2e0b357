#!/usr/bin/env python3
"""
bench_placement.py -- V contigs placed against the real phage matrix (tests/golden/ref_features.npz; contigs = negative rows,
cycled): the batched call (learning.place_contigs -> phk_placement_run) against the per-contig loop it replaces
(learning.kmeans + learning.cluster_silhouettes per contig, scripts/analysis.py:771-776), in the same process on the same
device.  Three repetitions each; wall time per contig, the kernels' hipEvent time split by stage (a separate profiled
run), launches, and the share of contigs the device declined.  The loop's cost per contig does
not depend on V, so it is timed on at most --loop-contigs contigs.  One JSON line per V.

Usage:  python tools/bench_placement.py [--v 1 20 256 2048] [--loop-contigs 20] [--chunk 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _lib, kmer, learning  # noqa: E402

STAGES = {"seed": ("pl_seed_dist_kernel", "pl_seed_choose_kernel", "pl_dup_kernel"),
          "lloyd": ("pl_assign_kernel", "pl_update_kernel", "pl_stop_kernel"),
          "silhouettes": ("pl_members_kernel", "pl_silhouette_kernel")}


def loop(pos, Z, k):
    out = []
    for z in Z:
        app = np.vstack((pos, z[None, :]))
        a = learning.kmeans(app, k)
        out.append((a, learning.cluster_silhouettes(app, a, a[-1])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--v", type=int, nargs="+", default=[1, 20, 256, 2048])
    ap.add_argument("--loop-contigs", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    with np.load(os.path.join(REPO, "tests", "golden", "ref_features.npz")) as z:
        pos = kmer.normalize_counts(z["pos_counts"].astype(np.int64))
        neg = kmer.normalize_counts(z["neg_counts"].astype(np.int64))
    k = 86
    ctx = _lib.get_context()
    learning.place_contigs(pos, neg[:2], k)      # warm-up: code objects, workspaces
    loop(pos, neg[:1], k)
    for V in args.v:
        Z = neg[np.arange(V) % neg.shape[0]]
        batched, routes = [], None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            recs = learning.place_contigs(pos, Z, k, _chunk=args.chunk)
            batched.append(time.perf_counter() - t0)
            routes = [r["route"] for r in recs]
        ctx.profile_enable(True)
        ctx.profile_reset()
        learning.place_contigs(pos, Z, k, _chunk=args.chunk)
        prof = ctx.profile()
        ctx.profile_enable(False)
        n_loop = min(V, args.loop_contigs)
        looped = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ref = loop(pos, Z[:n_loop], k)
            looped.append(time.perf_counter() - t0)
        same = all(np.array_equal(ref[i][0], recs[i]["labels"]) for i in range(n_loop))
        stage_ms = {s: sum(prof.get(n, (0.0, 0))[0] for n in names) for s, names in STAGES.items()}
        launches = int(sum(v[1] for n, v in prof.items() if n.startswith("pl_")))
        print(json.dumps({
            "V": V, "chunk": args.chunk, "batched_wall_s": batched, "batched_ms_per_contig": [1e3 * t / V for t in batched],
            "loop_contigs": n_loop, "loop_wall_s": looped, "loop_ms_per_contig": [1e3 * t / n_loop for t in looped],
            "speedup_best_vs_best": (min(looped) / n_loop) / (min(batched) / V),
            "speedup_worst_batched_vs_best_loop": (min(looped) / n_loop) / (max(batched) / V),
            "kernel_ms_by_stage": stage_ms, "kernel_ms_per_contig": sum(stage_ms.values()) / V, "launches": launches,
            "host_route_share": routes.count("host") / float(V), "labels_equal_to_loop": bool(same)}), flush=True)


if __name__ == "__main__":
    main()
