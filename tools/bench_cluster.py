#!/usr/bin/env python3
"""Clustering benchmark: learning.silhouettes and learning.dbscan on the device (phk_silhouettes, phk_dbscan) at 2^14 and
2^17 synthetic rows of D = 256 (normalised random profiles; silhouettes with 86 labels, DBSCAN at eps = 1, the reference's
default, where every pair is a neighbour and every point is core).  Reports seconds per call (host clock, the whole
host-pointer call with its transfers, median after a warm-up), the achieved fp64 rate (3 flops -- subtract, multiply, add --
per pair and column: 3 n^2 D for silhouettes, and for DBSCAN 3 n^2 D for the counts + 1.5 n^2 D for the symmetric union
pass), and the per-kernel times of the library's event timers.  --cpu also times scikit-learn at 2^14 rows.  One JSON line
per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="*", default=[1 << 14, 1 << 17])
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--labels", type=int, default=86)
ap.add_argument("--eps", type=float, default=1.0)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--cpu", action="store_true", help="also time scikit-learn at 2^14 rows")
a = ap.parse_args()

ctx = _lib.Context(0)


def timed(f):
    f()
    times = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        f()
        times.append(time.perf_counter() - t0)
    ctx.profile_reset()
    ctx.profile_enable(True)
    r = f()
    prof = {name: v[0] for name, v in ctx.profile().items()}
    ctx.profile_enable(False)
    return float(np.median(times)), times, prof, r


for n in a.rows:
    rng = np.random.default_rng(n)
    X = rng.random((n, a.dim))
    X /= X.sum(axis=1, keepdims=True)
    lab = rng.integers(0, a.labels, n).astype(np.uint32)
    s, ts, prof, out = timed(lambda: _lib.silhouettes(ctx, X, lab, a.labels))
    flop = 3.0 * n * n * a.dim
    print(json.dumps({"workload": "silhouettes", "rows": n, "dim": a.dim, "labels": a.labels, "s_per_call": s, "s_calls": ts,
                      "tflops": flop / s / 1e12, "kernel_tflops": flop / prof["phk_cl_silhouette_sums_kernel"] / 1e9,
                      "per_kernel_ms": prof, "mean_silhouette": float(out.mean())}), flush=True)
    s, ts, prof, out = timed(lambda: _lib.dbscan(ctx, X, a.eps, 2))
    flop = 4.5 * n * n * a.dim
    print(json.dumps({"workload": "dbscan", "rows": n, "dim": a.dim, "eps": a.eps, "min_samples": 2, "s_per_call": s,
                      "s_calls": ts, "tflops": flop / s / 1e12, "clusters": out[2], "core": int(out[1].sum()),
                      "count_kernel_tflops": 3.0 * n * n * a.dim / prof["phk_cl_count_kernel"] / 1e9,
                      "per_kernel_ms": prof}), flush=True)
    if a.cpu and n <= 1 << 14:
        from sklearn.cluster import DBSCAN
        from sklearn.metrics import silhouette_samples
        t0 = time.perf_counter()
        silhouette_samples(X, lab)
        t1 = time.perf_counter()
        DBSCAN(eps=a.eps, min_samples=2).fit(X[:1 << 12])      # (all-pairs neighbour lists: 2^12 rows only)
        t2 = time.perf_counter()
        print(json.dumps({"workload": "sklearn", "rows": n, "dim": a.dim, "silhouette_samples_s": t1 - t0,
                          "dbscan_rows": 1 << 12, "dbscan_s": t2 - t1}), flush=True)
ctx.close()
