#!/usr/bin/env python3
"""
bench_dbscan_sweep.py -- the DBSCAN parameter grid both ways in one process on one device: the batched sweep
(learning.dbscan_sweep -> phk_dbscan_sweep: the rows go up once, one pass over the pairs per stage for all cells) against
the loop it replaces (learning.dbscan_fit per cell: an upload, a count pass and a union pass per cell).

Row "phage": the 2255 phage rows of tests/golden/ref_features.npz over the 28 cells of tests/golden/dbscan_sweep.npz.
Row "synthetic": 16384 seeded blob rows, D = 256, 32 cells (8 eps x 4 min_samples).  One warm-up of each side, then --reps
timed repetitions: wall times, median and spread; a separate profiled run of each side gives the kernels' hipEvent time
and their shares.  One JSON line per row; the labels of both sides are compared.

Usage:  python tools/bench_dbscan_sweep.py [--reps 5] [--rows phage synthetic]
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


def loop(data, cells):
    return [learning.dbscan_fit(data, eps, m)[0] for eps, m in cells]


def blobs(rows, D, seed):
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-1, 1, (40, D))
    return centres[rng.randint(0, 40, rows)] + 0.25 * rng.randn(rows, D)


def stats(t):
    return {"wall_s": t, "median_s": float(np.median(t)), "min_s": min(t), "max_s": max(t)}


def profiled(ctx, fn):
    ctx.profile_enable(True)
    ctx.profile_reset()
    fn()
    prof = ctx.profile()
    ctx.profile_enable(False)
    total = sum(v[0] for v in prof.values())
    return {"kernel_ms": {n: round(v[0], 3) for n, v in prof.items()}, "launches": {n: int(v[1]) for n, v in prof.items()},
            "kernel_ms_total": round(total, 3),
            "share": {n: round(v[0] / total, 4) for n, v in prof.items()} if total else {}}


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
            with np.load(os.path.join(REPO, "tests", "golden", "dbscan_sweep.npz")) as g:
                eps_values, ms_values = g["eps_values"].tolist(), g["min_samples_values"].tolist()
        else:
            data = blobs(16384, 256, 7)
            eps_values, ms_values = [5.2, 5.4, 5.5, 5.6, 5.7, 5.8, 6.0, 6.4], [2, 5, 10, 20]
        cells = [(e, m) for e in eps_values for m in ms_values]
        learning.dbscan_sweep(data, eps_values[:1], ms_values[:1])          # warm-up: code objects, workspaces
        loop(data, cells[:1])
        swept, records = [], None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            records = learning.dbscan_sweep(data, eps_values, ms_values)
            swept.append(time.perf_counter() - t0)
        looped, ref = [], None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ref = loop(data, cells)
            looped.append(time.perf_counter() - t0)
        print(json.dumps({
            "row": row, "n": int(data.shape[0]), "D": int(data.shape[1]), "cells": len(cells), "sweep": stats(swept),
            "loop": stats(looped), "loop_over_sweep_median": float(np.median(looped) / np.median(swept)),
            "sweep_kernels": profiled(ctx, lambda: learning.dbscan_sweep(data, eps_values, ms_values)),
            "loop_kernels": profiled(ctx, lambda: loop(data, cells)),
            "n_clusters": [r["n_clusters"] for r in records],
            "labels_equal": bool(all(np.array_equal(r["labels"], l) for r, l in zip(records, ref)))}), flush=True)


if __name__ == "__main__":
    main()
