#!/usr/bin/env python3
"""Mixture sweep measurements, one JSON line.

grid   the two-class grid on the 2 255 + 2 418 reference rows of tests/golden/ref_features.npz: the validator's 20 folds,
       seed 0, K in --components.  ``mixture.cross_validate`` (all fits of the grid in lock step, one device call per EM
       iteration) against the same cells as a loop of ``mixture.fit`` and ``mixture.score``, in this process; the scores of
       the two are compared with array_equal.  Seconds by the host clock, per K for the loop; AUC and accuracy per K.
step   one ``_lib.MixtureSweep.step`` over J jobs (the grid's first J training cells, K = --step-components, at their
       start tables): milliseconds per call and per job (every J timed twice, in rising and in falling order of J, --steps
       calls each after warm-up: the median of all, the smallest and the largest), beside one ``MixtureTable.update`` +
       ``expect`` on the same rows, which is what an iteration of ``mixture.fit`` costs on the device side.
"""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _lib, cross_validate, likelihood, mixture

ap = argparse.ArgumentParser()
ap.add_argument("--components", type=int, nargs="*", default=[8, 32, 86, 256])
ap.add_argument("--folds", type=int, default=20)
ap.add_argument("--max-iter", type=int, default=50)
ap.add_argument("--jobs", type=int, nargs="*", default=[1, 40, 160])
ap.add_argument("--step-components", type=int, default=32)
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--skip-grid", action="store_true")
ap.add_argument("--skip-step", action="store_true")
a = ap.parse_args()

with np.load(os.path.join(REPO, "tests", "golden", "ref_features.npz")) as z:
    pos, neg = z["pos_counts"].astype(np.uint32), z["neg_counts"].astype(np.uint32)
ctx = _lib.get_context()
plan = cross_validate.FoldPlan(len(pos), len(neg), a.folds, 0)
out = {"workload": "mixture_sweep", "reference_rows": [len(pos), len(neg)], "folds": a.folds, "max_iter": a.max_iter}


def grid():
    mixture.fit(pos[:300], 4, seed=0, max_iter=2)                     # the library loaded, the workspaces warm
    t0 = time.perf_counter()
    res = mixture.cross_validate(pos, neg, a.components, a.folds, seed=0, fit_seed=0, max_iter=a.max_iter)
    sweep_s = time.perf_counter() - t0
    per_K, same = {}, True
    for b, K in enumerate(a.components):
        t0 = time.perf_counter()
        want, iters = np.full(len(pos) + len(neg), np.nan), []
        for f in range(a.folds):
            mp = mixture.fit(pos[plan.positive != f], K, seed=0, max_iter=a.max_iter)
            mn = mixture.fit(neg[plan.negative != f], K, seed=0, max_iter=a.max_iter)
            hp, hn = np.flatnonzero(plan.positive == f), np.flatnonzero(plan.negative == f)
            want[hp], want[len(pos) + hn] = mixture.score(pos[hp], mp, mn), mixture.score(neg[hn], mp, mn)
            iters += [mp.n_iter, mn.n_iter]
        loop_s = time.perf_counter() - t0
        same = same and bool(np.array_equal(want, res.scores[b]))
        per_K[str(K)] = {"loop_s": loop_s, "iterations": [int(min(iters)), int(max(iters))], "auc": float(res.auc[b]),
                         "accuracy": float(res.accuracy[b]), "dead": int(res.dead[b]),
                         "held_out_per_kmer": [float(res.held_out_per_kmer_positive[b]), float(res.held_out_per_kmer_negative[b])]}
    return {"sweep_s": sweep_s, "loop_s": sum(v["loop_s"] for v in per_K.values()), "scores_equal": same, "per_K": per_K}


def step():
    K, n_pos = a.step_components, len(pos)
    sets = ([np.flatnonzero(plan.positive != f) for f in range(a.folds)] +
            [n_pos + np.flatnonzero(plan.negative != f) for f in range(a.folds)])
    host = np.vstack((pos, neg))
    tables = []
    for j in range(max(a.jobs)):
        s = j % len(sets)
        rows = host[sets[s]]
        index = np.random.RandomState(j).choice(len(rows), K, replace=False)
        tables.append((s, likelihood.log_table(rows[index], 0.5), np.log(np.full(K, 1.0 / K))))
    res = {"components": K, "per_jobs": {}}
    dev = _lib.MixtureSweep(ctx, host, sets)
    try:
        dev.step(tables[:max(a.jobs)])                                # the workspace at its largest before any timing
        for J in a.jobs + a.jobs[::-1]:                               # every J twice, in both orders
            times = []
            for i in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                dev.step(tables[:J])
                if i >= a.warmup:
                    times.append(1e3 * (time.perf_counter() - t0))
            res["per_jobs"].setdefault(str(J), []).extend(times)
        for J, times in res["per_jobs"].items():
            ms = float(np.median(times))
            res["per_jobs"][J] = {"ms_per_call": ms, "ms_per_job": ms / int(J), "min_ms": min(times), "max_ms": max(times)}
    finally:
        dev.close()
    s, logp, logw = tables[0]
    batch = _lib.Batch.from_counts(ctx, host[sets[s]])
    table = _lib.MixtureTable(ctx, logp, logw)
    times = []
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        table.update(logp, logw)
        batch.mixture_expect(table)
        if i >= a.warmup:
            times.append(time.perf_counter() - t0)
    res["single_call_ms"] = 1e3 * float(np.median(times))
    table.close()
    batch.close()
    return res


if not a.skip_step:
    out["step"] = step()
if not a.skip_grid:
    out["grid"] = grid()
print(json.dumps(out))
