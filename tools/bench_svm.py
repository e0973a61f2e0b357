#!/usr/bin/env python3
"""svm scoring benchmark.  (1) The NuSVC fit on the full PhaMers 4-mer reference (2255 + 2418 rows, NuSVC() defaults):
ms per fit, solver iterations and us per iteration (fit time over iterations, the kernel matrix included).  (2) 2^20
resident synthetic 5 kb contigs (phk_synth_packed_dev), counted once, then scored count -> svm (phk_score_counts_dev):
ms per step (host clock around a device synchronise, after warm-up) and the fp64 TFLOP/s of the Gram product against the
support vectors (2 N n_sv D flops over the step).  Per-kernel times from the library's event timers; the kernel split of
a rocprofv3 run goes to profiles/svm/kernel_stats.csv."""
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
ap.add_argument("--fits", type=int, default=5)
a = ap.parse_args()

with np.load(os.path.join(REPO, "tests", "golden", "ref_features.npz")) as z:
    pos = z["pos_counts"].astype(np.float64)
    neg = z["neg_counts"].astype(np.float64)
pos /= pos.sum(axis=1, keepdims=True)
neg /= neg.sum(axis=1, keepdims=True)
ctx = _lib.Context(0)
X = np.vstack((pos, neg))
y = np.r_[np.ones(len(pos)), np.zeros(len(neg))]
gamma = _lib.svm_gamma(X, "scale")
fit_ms = []
for i in range(a.fits + 1):
    t0 = time.perf_counter()
    sup, coef, rho, n_iter = _lib.nusvc_fit(ctx, X, y, 0.5, gamma, 1e-3)
    if i:
        fit_ms.append((time.perf_counter() - t0) * 1e3)
ctx.profile_reset()
ctx.profile_enable(True)
_lib.nusvc_fit(ctx, X, y, 0.5, gamma, 1e-3)
ctx.sync()
fit_prof = {name: v[0] for name, v in ctx.profile().items()}
ctx.profile_enable(False)

model = _lib.Model(ctx, pos, neg, k_neighbors=3)
model.fit_svm()
n, L, k, D = a.contigs, a.length, 4, 256
T = n * L
packed = device.DeviceArray(ctx, device.packed_words(T), np.uint32)
off = device.DeviceArray(ctx, n + 1, np.uint64)
counts = device.DeviceArray(ctx, (n, D), np.uint32)
scores = device.DeviceArray(ctx, n, np.float64)
status = device.DeviceArray.from_host(ctx, np.zeros(1, np.uint32))
device.synth_packed(ctx, 0, 0, n, L, packed, off)
device.count(ctx, packed, None, T, off, n, k, counts)


def step():
    device.score_counts(ctx, model, counts, n, "svm", scores, status)


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
n_sv = len(sup)
gram = 2.0 * n * n_sv * D
fms = float(np.median(fit_ms))
print(json.dumps({"workload": "svm", "fit_ms": fms, "fit_ms_all": fit_ms, "n_iter": n_iter, "n_sv": n_sv,
                  "us_per_iter": fms * 1e3 / n_iter, "fit_per_kernel_ms": fit_prof,
                  "contigs": n, "length": L, "k": k, "ms_per_step": ms, "ms_steps": times, "queries_per_s": n / ms * 1e3,
                  "gram_tflops": gram / ms / 1e9, "gram_tflop": gram / 1e12,
                  "partial_kernel_tflops": gram / prof.get("phk_svm_partial_kernel", float("nan")) / 1e9,
                  "per_kernel_ms": prof, "nan_rows": int(status.to_host()[0]), "fraction_positive": float(np.mean(s))}))
