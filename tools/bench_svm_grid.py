#!/usr/bin/env python3
"""
bench_svm_grid.py -- what the NuSVC nu x gamma sweep (svm.nusvc_sweep, phk_nusvc_sweep) costs against the loop of
svm.NuSVC(...).fit + decision_function calls it replaces (profiles/svm_grid/README.md).  The loop is the baseline; the sweep
is never its own baseline.

The grid: 6 gammas ('scale' x 1/16 .. 2 in doublings) x 6 nus (0.1 .. 0.6) on the reference rows (tests/golden/
ref_features.npz, 2 255 + 2 418 rows), 5 folds, seed 0: 216 fits and 180 held-out decision calls.

  (a) wall time of the sweep and of the loop, --repeats runs each, ALTERNATING (sweep, loop, sweep, loop, ...) after --warmup
      untimed rounds; the spread of each is printed beside its median.
  (b) kernel time of one profiled run of each (the context's event timers, a run of its own), per kernel name with launch
      counts, and the time per solver iteration they imply: the sweep's solver kernel time over the iterations of the longest
      problem of each launch chain (problems run side by side), the single solver's kernel time over all its iterations.
  (c) the table: auc, accuracy, n_support and n_iter per cell, the best cell and the default cell (gamma 'scale', nu 0.5).
  (d) the sweep at other workgroup sizes and with the state in global memory (kernel time of the solver only).

Both sides are checked to give the same held-out decisions before anything is timed.  One JSON line per measurement.

Usage:  python tools/bench_svm_grid.py [--repeats 3] [--warmup 1] [--folds 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def profiled(ctx, fn):
    """{kernel name: [ms, launches]} of one profiled run of fn, the svm kernels and the row norms."""
    ctx.profile_enable(True)
    ctx.profile_reset()
    fn()
    ctx.sync()
    prof = ctx.profile()
    ctx.profile_enable(False)
    return {name: [round(ms, 3), int(cnt)] for name, (ms, cnt) in prof.items() if "svm" in name or "rownorm" in name}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--folds', type=int, default=5)
    args = ap.parse_args()
    from phamers_amd import _lib, cross_validate, kmer, svm
    ctx = _lib.get_context()
    with np.load(os.path.join(REPO, 'tests', 'golden', 'ref_features.npz')) as z:
        pos = kmer.normalize_counts(z['pos_counts'].astype(np.int64))
        neg = kmer.normalize_counts(z['neg_counts'].astype(np.int64))
    X = np.ascontiguousarray(np.vstack((pos, neg)))
    y = np.r_[np.ones(len(pos)), np.zeros(len(neg))]
    scale = _lib.svm_gamma(X, 'scale')
    gammas = [scale * 2.0 ** e for e in range(-4, 2)]
    nus = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
    N, seed = args.folds, 0
    plan = cross_validate.FoldPlan(len(pos), len(neg), N, seed)
    fold_of = np.r_[plan.positive, plan.negative]

    def sweep(**kw):
        return svm.nusvc_sweep(X, y, nus, gammas, folds=N, seed=seed, **kw)

    def loop():
        """The same problems one by one: (n_iter of every fit (Gm, V, N + 1), held-out decisions (Gm, V, n))."""
        iters = np.zeros((len(gammas), len(nus), N + 1), dtype=np.int64)
        dec = np.full((len(gammas), len(nus), len(y)), np.nan)
        for g, gamma in enumerate(gammas):
            for v, nu in enumerate(nus):
                iters[g, v, 0] = svm.NuSVC(nu=nu, gamma=gamma).fit(X, y).n_iter_[0]
                for f in range(N):
                    held = fold_of == f
                    m = svm.NuSVC(nu=nu, gamma=gamma).fit(X[~held], y[~held])
                    iters[g, v, f + 1] = m.n_iter_[0]
                    dec[g, v, held] = m.decision_function(X[held])
        return iters, dec

    # the same numbers from both sides, before any timing (this is also the first warm-up round)
    res = sweep()
    iters, dec = loop()
    assert (res.status == 0).all(), res.status
    same = bool(np.array_equal(res.held_decision, dec) and np.array_equal(res.n_iter, iters[:, :, 0])
                and np.array_equal(res.fold_n_iter, iters[:, :, 1:]))
    print(json.dumps({"case": "check", "sweep_equals_loop_bit_for_bit": same, "fits": int(iters.size),
                      "iterations_total": int(iters.sum()), "iterations_longest_fit": int(iters.max())}))
    if not same:
        return 1

    # (a) wall, alternating
    for _ in range(max(args.warmup - 1, 0)):
        sweep()
        loop()
    t_s, t_l = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        sweep()
        t_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        loop()
        t_l.append(time.perf_counter() - t0)
    ms = lambda t: [round(x * 1e3, 1) for x in t]   # noqa: E731
    print(json.dumps({"case": "a", "sweep_ms": round(float(np.median(t_s)) * 1e3, 1), "loop_ms": round(float(np.median(t_l)) * 1e3, 1),
                      "sweep_runs": ms(t_s), "loop_runs": ms(t_l),
                      "sweep_spread_ms": round((max(t_s) - min(t_s)) * 1e3, 1), "loop_spread_ms": round((max(t_l) - min(t_l)) * 1e3, 1),
                      "ratio_loop_over_sweep": round(float(np.median(t_l) / np.median(t_s)), 2)}))

    # (b) kernels
    ks, kl = profiled(ctx, sweep), profiled(ctx, loop)
    # a launch chain of the sweep runs until its longest problem stops: iterations on the critical path, per pass of gammas
    crit = int(iters.max())   # (one pass holds every gamma of this grid: 6 x 87 MB of kernel matrices)
    print(json.dumps({"case": "b", "sweep_kernels": ks, "loop_kernels": kl,
                      "sweep_solver_us_per_iteration_of_the_longest_fit": round(ks["phk_svm_sweep_solve_kernel"][0] * 1e3 / crit, 2),
                      "sweep_solver_us_per_iteration_over_all_fits": round(ks["phk_svm_sweep_solve_kernel"][0] * 1e3 / iters.sum(), 3),
                      "single_solver_us_per_iteration": round(kl["phk_svm_solve_kernel"][0] * 1e3 / iters.sum(), 2)}))

    # (c) the table
    best = np.unravel_index(int(np.nanargmax(res.auc)), res.auc.shape)
    dflt = (gammas.index(scale), nus.index(0.5))
    print(json.dumps({"case": "c", "gammas": gammas, "gamma_over_scale": [2.0 ** e for e in range(-4, 2)], "nus": nus,
                      "auc": np.round(res.auc, 5).tolist(), "accuracy": np.round(res.accuracy, 5).tolist(),
                      "n_support": res.n_support.tolist(), "n_iter": res.n_iter.tolist()}))
    for name, (g, v) in (("best", best), ("default", dflt)):
        print(json.dumps({"case": "c", "cell": name, "gamma": gammas[g], "gamma_over_scale": gammas[g] / scale, "nu": nus[v],
                          "auc": float(res.auc[g, v]), "accuracy": float(res.accuracy[g, v]),
                          "n_support": int(res.n_support[g, v]), "n_iter": int(res.n_iter[g, v])}))

    # (d) the solver at other shapes
    for label, kw in (("lds_default", {}), ("lds_1024", {"_threads": 1024}), ("lds_512", {"_threads": 512}),
                      ("lds_256", {"_threads": 256}), ("global_default", {"_lds_rows": 0}),
                      ("global_1024", {"_lds_rows": 0, "_threads": 1024})):
        runs = [profiled(ctx, lambda: sweep(**kw))["phk_svm_sweep_solve_kernel"][0] for _ in range(2)]
        print(json.dumps({"case": "d", "solver": label, "solve_kernel_ms": runs,
                          "us_per_iteration_of_the_longest_fit": round(min(runs) * 1e3 / crit, 2)}))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
