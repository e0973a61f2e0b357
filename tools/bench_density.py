#!/usr/bin/env python3
"""Density scoring benchmark: 2^20 resident synthetic 5 kb contigs (phamers_amd.synth / phk_synth_packed_dev), counted once,
then scored count -> density (phk_score_counts_dev) against the full PhaMers 4-mer reference (2255 + 2418 rows, not
equalised).  Reports ms per scoring step (host clock around a device synchronise, after warm-up), queries/s, the fp64
TFLOP/s of the Gram product (2 N M D flops over the step), and the per-kernel times of the library's event timers."""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _lib, device

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=1 << 20)
ap.add_argument("--length", type=int, default=5000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--fused", action="store_true", help="time phk_count_score_dev (count + density) instead of scoring alone")
a = ap.parse_args()

with np.load(os.path.join(REPO, "tests", "golden", "ref_features.npz")) as z:
    pos = z["pos_counts"].astype(np.float64)
    neg = z["neg_counts"].astype(np.float64)
pos /= pos.sum(axis=1, keepdims=True)
neg /= neg.sum(axis=1, keepdims=True)
ctx = _lib.Context(0)
model = _lib.Model(ctx, pos, neg, k_neighbors=3)
n, L, k, D = a.contigs, a.length, 4, 256
M = pos.shape[0] + neg.shape[0]
T = n * L
packed = device.DeviceArray(ctx, device.packed_words(T), np.uint32)
off = device.DeviceArray(ctx, n + 1, np.uint64)
counts = device.DeviceArray(ctx, (n, D), np.uint32)
scores = device.DeviceArray(ctx, n, np.float64)
status = device.DeviceArray.from_host(ctx, np.zeros(1, np.uint32))
device.synth_packed(ctx, 0, 0, n, L, packed, off)
device.count(ctx, packed, None, T, off, n, k, counts)


def step():
    if a.fused:
        device.count_score(ctx, model, packed, None, T, off, n, k, "density", counts, scores, status)
    else:
        device.score_counts(ctx, model, counts, n, "density", scores, status)


for _ in range(a.warmup):
    step()
ctx.sync()
times = []
for _ in range(a.steps):
    t0 = time.perf_counter()
    step()
    ctx.sync()
    times.append((time.perf_counter() - t0) * 1e3)
ctx.profile_reset()
ctx.profile_enable(True)
step()
ctx.sync()
prof = {name: v[0] for name, v in ctx.profile().items()}
ctx.profile_enable(False)
ms = float(np.median(times))
s = scores.to_host()
gram = 2.0 * n * M * D
print(json.dumps({"workload": "density", "contigs": n, "length": L, "k": k, "reference_rows": M, "fused_count": a.fused,
                  "ms_per_step": ms, "ms_steps": times, "queries_per_s": n / ms * 1e3,
                  "gram_tflops": gram / ms / 1e9, "gram_tflop": gram / 1e12,
                  "partial_kernel_tflops": gram / prof.get("phk_kde_partial_kernel", float("nan")) / 1e9,
                  "per_kernel_ms": prof, "nan_rows": int(status.to_host()[0]),
                  "score_mean": float(np.mean(s)), "score_min": float(np.min(s)), "score_max": float(np.max(s))}))
