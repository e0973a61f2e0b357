#!/usr/bin/env python3
"""Nearest-reference lookup benchmark: resident synthetic 5 kb contigs (2^20 by default) against the full PhaMers 4-mer
reference (2255 + 2418 rows), k = 1, 5, 28.  Times Batch.neighbors (host clock around the call, which ends with the result
on the host; median after warm-up), and reports the fallback share and the per-kernel times of the library's event timers.

--baseline times what a user can do without the lookup (it runs on a tree that lacks it): phk_distances in row blocks,
the dense block brought to the host, np.argpartition and np.lexsort there -- on --baseline-rows contigs, scaled to the
whole batch (the cost is linear in the rows)."""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _lib, device

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=1 << 20)
ap.add_argument("--length", type=int, default=5000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--k", type=int, nargs="+", default=[1, 5, 28])
ap.add_argument("--baseline", action="store_true")
ap.add_argument("--baseline-rows", type=int, default=1 << 14)
a = ap.parse_args()

with np.load(os.path.join(REPO, "tests", "golden", "ref_features.npz")) as z:
    pos = z["pos_counts"].astype(np.float64)
    neg = z["neg_counts"].astype(np.float64)
pos /= pos.sum(axis=1, keepdims=True)
neg /= neg.sum(axis=1, keepdims=True)
ctx = _lib.Context(0)
n, L, k4, D = a.contigs, a.length, 4, 256
M = pos.shape[0] + neg.shape[0]
T = n * L
packed = device.DeviceArray(ctx, device.packed_words(T), np.uint32)
off = device.DeviceArray(ctx, n + 1, np.uint64)
counts = device.DeviceArray(ctx, (n, D), np.uint32)
device.synth_packed(ctx, 0, 0, n, L, packed, off)
device.count(ctx, packed, None, T, off, n, k4, counts)
host_counts = counts.to_host()
del packed, counts


def median_ms(fn):
    for _ in range(a.warmup):
        fn()
    times = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), times


if a.baseline:
    X = np.ascontiguousarray(np.vstack((pos, neg)))
    rows = min(n, a.baseline_rows)
    Q = host_counts[:rows].astype(np.float64)
    Q /= Q.sum(axis=1, keepdims=True)
    for k in a.k:
        def host_way():
            idx, dist = np.empty((rows, k), np.int64), np.empty((rows, k))
            for s in range(0, rows, 4096):
                q = np.ascontiguousarray(Q[s:s + 4096])
                d = np.empty((q.shape[0], M))
                _lib.check(ctx.lib.phk_distances(ctx.handle, _lib.ptr(q), q.shape[0], _lib.ptr(X), M, D, _lib.ptr(d)))
                part = np.argpartition(d, k - 1, axis=1)[:, :k] if k < M else np.tile(np.arange(M), (q.shape[0], 1))
                pd = np.take_along_axis(d, part, axis=1)
                for r in range(q.shape[0]):          # (ties at the cut are not resolved by index here: a user would not either)
                    o = np.lexsort((part[r], pd[r]))
                    idx[s + r], dist[s + r] = part[r][o], pd[r][o]
            return idx, dist
        ms, times = median_ms(host_way)
        print(json.dumps({"workload": "neighbors_baseline", "contigs": n, "timed_rows": rows, "k": k, "reference_rows": M,
                          "ms_timed_rows": ms, "ms_steps": times, "ms_scaled_to_contigs": ms * n / rows,
                          "dense_bytes_over_the_bus": n * M * 8}))
    sys.exit(0)

model = _lib.Model(ctx, pos, neg, k_neighbors=3)
batch = _lib.Batch.from_counts(ctx, host_counts)
del host_counts
for k in a.k:
    ctx.neighbors_stats()
    ms, times = median_ms(lambda: batch.neighbors(model, k))
    queries, fell = ctx.neighbors_stats()
    ctx.profile_reset()
    ctx.profile_enable(True)
    dist, idx = batch.neighbors(model, k)
    ctx.sync()
    prof = {name: v[0] for name, v in ctx.profile().items()}
    ctx.profile_enable(False)
    ctx.neighbors_stats()
    print(json.dumps({"workload": "neighbors", "contigs": n, "length": L, "k": k, "reference_rows": M, "ms_per_call": ms,
                      "ms_steps": times, "queries_per_s": n / ms * 1e3, "fallback_share": fell / max(queries, 1),
                      "per_kernel_ms": prof, "partial_over_kde_partial_64_6ms_per_2p20": prof.get("phk_nn_partial_kernel", float("nan")) / (64.6 * n / (1 << 20)),
                      "mean_nearest_distance": float(dist[:, 0].mean())}))
