#!/usr/bin/env python3
"""
bench_combo_grid.py -- what the k_neighbors x k_clusters grid (combo_grid.sweep, phk_combo_grid) costs against the loop of
cross_validator runs it replaces (profiles/combo_grid/README.md).  The loop is the baseline; the sweep is never its own
baseline.

The grid: 6 k_neighbors (1, 3, 5, 7, 9, 15) x 8 k_clusters (10, 20, 40, 60, 86, 120, 160, 200) on the reference rows
(tests/golden/ref_features.npz, 2 255 + 2 418 rows), 20 folds, seed 0.  The loop is one cross_validator run per number of the
table: method 'combo' for every cell (48 runs), 'knn' per k_neighbors (6) and 'kmeans' per k_clusters (8), each on the
validator's default paths (its per-fold fit is learning.kmeans, its scoring route the model's own).

  (a) wall time of the sweep (--repeats runs, one before the loop and the rest after it) and of the loop (one run: it takes
      minutes), after one untimed sweep; the sweep's seconds per stage beside it.
  (b) kernel time of one profiled sweep (the context's event timers, a run of its own) per kernel name with launch counts.
  (c) the table: knn_auc, kmeans_auc, auc, accuracy per cell, the best cell and the default cell (3, 86).

Both sides are compared before the figures are printed: votes equal, the k-means half within 4 D 2^-53 (the validator's
default route at D = 256 sums its final distances in another order).  One JSON line per measurement.

Usage:  python tools/bench_combo_grid.py [--repeats 3] [--folds 20] [--loop_runs all|N]
        (--loop_runs N: only the first N validator runs of the loop, for a rehearsal; the printed line says so)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K_NEIGHBORS = (1, 3, 5, 7, 9, 15)
K_CLUSTERS = (10, 20, 40, 60, 86, 120, 160, 200)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--folds', type=int, default=20)
    ap.add_argument('--loop_runs', default='all')
    args = ap.parse_args()
    from phamers_amd import _lib, combo_grid, cross_validate, kmer
    ctx = _lib.get_context()
    with np.load(os.path.join(REPO, 'tests', 'golden', 'ref_features.npz')) as z:
        pos = kmer.normalize_counts(z['pos_counts'].astype(np.int64))
        neg = kmer.normalize_counts(z['neg_counts'].astype(np.int64))
    N, seed = args.folds, 0

    def sweep(details=None):
        return combo_grid.sweep(pos, neg, K_NEIGHBORS, K_CLUSTERS, N, seed=seed, _details=details)

    runs = [("combo", kn, kc) for kn in K_NEIGHBORS for kc in K_CLUSTERS] + [("knn", kn, 86) for kn in K_NEIGHBORS] + \
           [("kmeans", 3, kc) for kc in K_CLUSTERS]
    if args.loop_runs != 'all':
        runs = runs[:int(args.loop_runs)]

    def loop():
        """{(method, k_neighbors, k_clusters): (scores in vstack order, auc)} of one validator run each."""
        out, t_first = {}, time.perf_counter()
        for method, kn, kc in runs:
            v = cross_validate.cross_validator()
            v.positive_data, v.negative_data, v.method, v.N, v.seed = pos, neg, method, N, seed
            v.k_neighbors, v.k_clusters = kn, kc
            ps, ns = v.cross_validate()
            out[(method, kn, kc)] = (np.concatenate((ps, ns)), v.performance()[2])
            print("loop: %d of %d validator runs after %.1f s" % (len(out), len(runs), time.perf_counter() - t_first), file=sys.stderr,
                  flush=True)
        return out

    sweep()                                  # untimed: code objects, workspaces
    t_s, stages = [], []
    for r in range(args.repeats):
        if r == 1:
            t0 = time.perf_counter()
            looped = loop()
            ctx.sync()
            t_l = time.perf_counter() - t0
        d = {}
        t0 = time.perf_counter()
        res = sweep(d)
        ctx.sync()
        t_s.append(time.perf_counter() - t0)
        stages.append({k: round(v * 1e3, 1) for k, v in d["seconds"].items()})
    if args.repeats < 2:
        t0 = time.perf_counter()
        looped = loop()
        ctx.sync()
        t_l = time.perf_counter() - t0

    # the same numbers from both sides
    bound = 4 * pos.shape[1] * 2.0 ** -53
    votes_equal, worst, auc_gap = True, 0.0, 0.0
    for (method, kn, kc), (scores, auc) in looped.items():
        i, j = K_NEIGHBORS.index(kn), K_CLUSTERS.index(kc)
        knn, km = res.knn_scores[i], res.kmeans_scores[j]
        if method == "knn":
            votes_equal &= bool(np.array_equal(scores, knn))
            auc_gap = max(auc_gap, abs(auc - res.knn_auc[i]))
        elif method == "kmeans":
            worst = max(worst, float(np.abs(scores - km).max()))
            auc_gap = max(auc_gap, abs(auc - res.kmeans_auc[j]))
        else:
            votes_equal &= bool(np.array_equal(np.round(scores - km), knn))
            worst = max(worst, float(np.abs(scores - (knn + km)).max()))
            auc_gap = max(auc_gap, abs(auc - res.combo_auc[i, j]))
    ok = votes_equal and worst <= bound
    print(json.dumps({"case": "check", "validator_runs": len(runs), "votes_equal": votes_equal, "kmeans_half_largest_deviation": worst,
                      "allowed": bound, "largest_auc_difference": auc_gap, "host_routes": res.routes.count("host"),
                      "kmeans_problems": len(res.routes)}))
    if not ok:
        return 1

    ms = lambda t: [round(x * 1e3, 1) for x in t]   # noqa: E731
    print(json.dumps({"case": "a", "sweep_ms": round(float(np.median(t_s)) * 1e3, 1), "loop_ms": round(t_l * 1e3, 1),
                      "sweep_runs": ms(t_s), "sweep_spread_ms": round((max(t_s) - min(t_s)) * 1e3, 1),
                      "loop_validator_runs": len(runs), "loop_is_whole": args.loop_runs == 'all',
                      "ratio_loop_over_sweep": round(t_l / float(np.median(t_s)), 2), "sweep_stage_ms": stages}))

    ctx.profile_enable(True)
    ctx.profile_reset()
    sweep()
    ctx.sync()
    prof = ctx.profile()
    ctx.profile_enable(False)
    print(json.dumps({"case": "b", "sweep_kernels": {name: [round(t, 3), int(cnt)] for name, (t, cnt) in sorted(prof.items())}}))

    print(json.dumps({"case": "c", "k_neighbors": list(K_NEIGHBORS), "k_clusters": list(K_CLUSTERS),
                      "knn_auc": np.round(res.knn_auc, 5).tolist(), "kmeans_auc": np.round(res.kmeans_auc, 5).tolist(),
                      "auc": np.round(res.combo_auc, 5).tolist(), "accuracy": np.round(res.combo_accuracy, 5).tolist()}))
    best = np.unravel_index(int(np.argmax(res.combo_auc)), res.combo_auc.shape)
    for name, (i, j) in (("best", best), ("default", (K_NEIGHBORS.index(3), K_CLUSTERS.index(86)))):
        print(json.dumps({"case": "c", "cell": name, "k_neighbors": K_NEIGHBORS[i], "k_clusters": K_CLUSTERS[j],
                          "knn_auc": float(res.knn_auc[i]), "kmeans_auc": float(res.kmeans_auc[j]),
                          "auc": float(res.combo_auc[i, j]), "accuracy": float(res.combo_accuracy[i, j])}))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
