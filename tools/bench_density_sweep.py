#!/usr/bin/env python3
"""
bench_density_sweep.py -- what the density bandwidth sweep (learning.density_sweep, phk_kde_sweep) costs against the loop of
learning.log_density calls it replaces (profiles/density_sweep/README.md).  The loop is the baseline in every case; the
sweep is never its own baseline.

  (a) the 11 x 11 leave-one-out bandwidth grid on the reference rows (tests/golden/ref_features.npz, 2 255 + 2 418 rows):
      bandwidth.held_out_log_densities (four sweeps of 11 bandwidths) against the 44 log_density calls over the same pairs.
  (b) 2^17 synthetic queries x 4 673 rows at B = 1, NB, 2 NB and 16 bandwidths: one sweep against B log_density calls.
  (c) kernel time of one pass at 1 .. NB bandwidths (the context's kernel timers, a run of its own): where the exps stop
      hiding under the Gram.

Wall times are medians of --repeats timed runs after --warmup untimed ones; kernel times are event times summed per kernel
name.  One JSON line per measurement.

Usage:  python tools/bench_density_sweep.py [--repeats 5] [--warmup 2] [--queries 131072]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def median_wall(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3, [round(t * 1e3, 3) for t in times]


def kernel_ms(ctx, fn, prefix):
    """{kernel name: ms} of one profiled run of fn, kernels whose name starts with ``prefix``."""
    ctx.profile_enable(True)
    ctx.profile_reset()
    fn()
    ctx.sync()
    prof = ctx.profile()
    ctx.profile_enable(False)
    return {name: round(ms, 4) for name, (ms, _) in prof.items() if name.startswith(prefix)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--queries', type=int, default=1 << 17)
    args = ap.parse_args()
    from phamers_amd import _lib, bandwidth, kmer, learning
    ctx = _lib.get_context()
    NB = learning.DENSITY_SWEEP_PER_PASS
    with np.load(os.path.join(REPO, 'tests', 'golden', 'ref_features.npz')) as z:
        pos = kmer.normalize_counts(z['pos_counts'].astype(np.int64))
        neg = kmer.normalize_counts(z['neg_counts'].astype(np.int64))
    rows = np.ascontiguousarray(np.vstack((pos, neg)))

    # (a) the 11 x 11 leave-one-out grid
    hs = [0.002, 0.003, 0.004, 0.005, 0.006, 0.007, 0.008, 0.01, 0.012, 0.015, 0.02]

    def grid_sweep():
        return bandwidth.held_out_log_densities(pos, neg, hs, hs)

    def grid_loop():
        for q, x in ((pos, pos), (neg, pos), (pos, neg), (neg, neg)):
            for h in hs:
                learning.log_density(q, x, h)

    ms_s, runs_s = median_wall(grid_sweep, args.warmup, args.repeats)
    ms_l, runs_l = median_wall(grid_loop, args.warmup, args.repeats)
    print(json.dumps({"case": "a", "what": "11 x 11 leave-one-out grid, densities only", "sweep_ms": round(ms_s, 3),
                      "loop_ms": round(ms_l, 3), "sweep_runs": runs_s, "loop_runs": runs_l,
                      "sweep_kernels": kernel_ms(ctx, grid_sweep, "phk_kde"), "loop_kernels": kernel_ms(ctx, grid_loop, "phk_kde")}))
    t0 = time.perf_counter()
    table = bandwidth.grid(pos, neg, hs, hs)
    best = table["best"]
    print(json.dumps({"case": "a", "what": "grid() with its 121 device ROC areas", "ms": round((time.perf_counter() - t0) * 1e3, 1),
                      "best": [table["positive_bandwidth"][best], table["negative_bandwidth"][best], table["auc"][best]]}))
    for hp, hn in ((0.005, 0.01), (0.005, 0.005), (0.003, 0.003), (0.004, 0.003)):
        cell = hs.index(hp) * len(hs) + hs.index(hn)
        print(json.dumps({"case": "a", "cell": [hp, hn], "leave_one_out_auc": table["auc"][cell]}))
    print(json.dumps({"case": "a", "bandwidths": hs, "loglik_positive": table["loglik_positive"].tolist(),
                      "loglik_negative": table["loglik_negative"].tolist()}))
    folds = bandwidth.grid(pos, neg, [0.003, 0.004, 0.005], [0.003, 0.005, 0.01], folds=20, seed=0)
    print(json.dumps({"case": "a", "what": "20 folds, seed 0", "positive_bandwidth": folds["positive_bandwidth"].tolist(),
                      "negative_bandwidth": folds["negative_bandwidth"].tolist(), "auc": folds["auc"].tolist()}))

    # (b) 2^17 synthetic queries: mixtures of two reference rows
    rng = np.random.default_rng(0)
    i, j = rng.integers(0, len(rows), args.queries), rng.integers(0, len(rows), args.queries)
    w = rng.random(args.queries)[:, None]
    Q = np.ascontiguousarray(w * rows[i] + (1.0 - w) * rows[j])
    pool = [0.005, 0.01, 0.003, 0.02, 0.004, 0.007, 0.002, 0.015, 0.006, 0.03, 0.008, 0.012, 0.0025, 0.05, 0.009, 0.1]
    for B in sorted(set((1, NB, 2 * NB, 16))):
        hb = pool[:B]
        sweep = lambda: learning.density_sweep(Q, rows, hb)                    # noqa: E731
        loop = lambda: [learning.log_density(Q, rows, h) for h in hb]          # noqa: E731
        ms_s, runs_s = median_wall(sweep, args.warmup, args.repeats)
        ms_l, runs_l = median_wall(loop, args.warmup, args.repeats)
        print(json.dumps({"case": "b", "B": B, "queries": args.queries, "rows": len(rows), "sweep_ms": round(ms_s, 3),
                          "loop_ms": round(ms_l, 3), "sweep_runs": runs_s, "loop_runs": runs_l,
                          "sweep_kernels": kernel_ms(ctx, sweep, "phk_kde"), "loop_kernels": kernel_ms(ctx, loop, "phk_kde")}))

    # (c) kernel time of one pass against the number of bandwidths it carries
    for B in range(1, NB + 1):
        hb = pool[:B]
        runs = [kernel_ms(ctx, lambda: learning.density_sweep(Q, rows, hb), "phk_kde_sweep_partial") for _ in range(3)]
        ms = float(np.median([sum(r.values()) for r in runs]))
        print(json.dumps({"case": "c", "B": B, "partial_kernel_ms": round(ms, 4)}))
    one = [kernel_ms(ctx, lambda: learning.log_density(Q, rows, pool[0]), "phk_kde_partial") for _ in range(3)]
    print(json.dumps({"case": "c", "what": "phk_kde_partial_kernel, one bandwidth (the loop's kernel)",
                      "partial_kernel_ms": round(float(np.median([sum(r.values()) for r in one])), 4)}))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
