#!/usr/bin/env python3
"""
bench_sweep.py -- the silhouette-against-k study of scripts/cluster.py:31-47, both ways in one process on one device:
the batched sweep (cluster.silhouette_curve -> learning.kmeans_sweep -> phk_sweep_run) against the loop it replaces
(learning.kmeans, then learning.silhouette_score, per k: the single-problem paths, host seeding and one pair pass per k).

Row "phage": the 2255 phage rows of tests/golden/ref_features.npz over the reference's grid k = 10, 20, ..., 590.
Row "synthetic": 16384 seeded blob rows, D = 256, twelve values of k -- what the shared pair pass buys against twelve
phk_silhouettes calls.  One warm-up of each side, then --reps timed repetitions: wall times, median and spread; a separate
profiled run gives the kernels' hipEvent time by stage and the launch counts; the routes say how many problems the device
declined.  One JSON line per row.

Usage:  python tools/bench_sweep.py [--reps 5] [--rows phage synthetic]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _lib, cluster, kmer, learning  # noqa: E402

STAGES = {"seed": ("sw_seed_dist_kernel", "sw_seed_choose_kernel"),
          "lloyd": ("sw_assign_kernel", "sw_update_kernel", "sw_stop_kernel"),
          "silhouettes": ("sw_pair_kernel", "sw_silhouette_kernel", "phk_cl_silhouette_sums_kernel",
                          "phk_cl_silhouette_finish_kernel")}


def loop(data, ks):
    return np.array([learning.silhouette_score(data, learning.kmeans(data, int(k))) for k in ks])


def blobs(rows, D, seed):
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-1, 1, (40, D))
    return centres[rng.randint(0, 40, rows)] + 0.25 * rng.randn(rows, D)


def stats(t):
    return {"wall_s": t, "median_s": float(np.median(t)), "min_s": min(t), "max_s": max(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", nargs="+", default=["phage", "synthetic"])
    args = ap.parse_args()
    ctx = _lib.get_context()
    for row in args.rows:
        if row == "phage":
            with np.load(os.path.join(REPO, "tests", "golden", "ref_features.npz")) as z:
                data = kmer.normalize_counts(z["pos_counts"].astype(np.int64))
            ks = np.arange(10, 600, 10)
        else:
            data = blobs(16384, 256, 7)
            ks = np.array([2, 4, 8, 12, 16, 24, 32, 40, 48, 64, 96, 128])
        cluster.silhouette_curve(data, ks[:2])          # warm-up: code objects, workspaces
        loop(data, ks[:1])
        swept, curve = [], None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            curve = cluster.silhouette_curve(data, ks)
            swept.append(time.perf_counter() - t0)
        ctx.profile_enable(True)
        ctx.profile_reset()
        recs = learning.kmeans_sweep(data, ks)
        prof = ctx.profile()
        ctx.profile_enable(False)
        looped, ref = [], None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ref = loop(data, ks)
            looped.append(time.perf_counter() - t0)
        stage_ms = {s: sum(prof.get(n, (0.0, 0))[0] for n in names) for s, names in STAGES.items()}
        launches = {n: int(v[1]) for n, v in prof.items()}
        print(json.dumps({
            "row": row, "n": int(data.shape[0]), "D": int(data.shape[1]), "k_values": len(ks), "sweep": stats(swept),
            "loop": stats(looped), "loop_over_sweep_median": float(np.median(looped) / np.median(swept)),
            "kernel_ms_by_stage": stage_ms, "launches": launches, "launches_total": int(sum(launches.values())),
            "host_route_problems": [r["route"] for r in recs].count("host"),
            "max_abs_difference_of_the_curves": float(np.max(np.abs(curve[1] - ref)))}), flush=True)


if __name__ == "__main__":
    main()
