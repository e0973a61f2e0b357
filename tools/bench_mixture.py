#!/usr/bin/env python3
"""Mixture-of-multinomials measurements, one JSON line.

speed        2^20 resident synthetic 5 kb contigs (counted once on the device), D = 256, K in --components: ms per E-step
             (Batch.mixture_expect: both products, the fold, T / N_k / L back; host clock, median after warm-up), per EM
             iteration of mixture.fit (a fit at 2 and at 6 M-steps, the difference divided by 4), the kernels' event times
             and their fp64 rates, the NumPy float64 statement on the host over ``--numpy-rows`` of the contigs scaled to the
             batch, and one likelihood call (4 673 components, no weights) on the same rows in the same process.
compression  the validator's 20 folds, seed 0, on the 2 255 + 2 418 reference rows: K components fitted per class on each
             fold's training rows, the held-out rows scored with mixture.score -- as they are and thinned to n k-mers -- beside
             the one-component-per-row likelihood method on the same rows.  AUC and accuracy at threshold 0.
"""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _lib, cross_validate, device, likelihood, mixture

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=1 << 20)
ap.add_argument("--length", type=int, default=5000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--numpy-rows", type=int, default=4096)
ap.add_argument("--components", type=int, nargs="*", default=[16, 64, 256])
ap.add_argument("--folds", type=int, default=20)
ap.add_argument("--fit-components", type=int, nargs="*", default=[8, 32, 86, 256])
ap.add_argument("--lengths", type=int, nargs="*", default=[200, 500, 1000, 2000, 5000])
ap.add_argument("--max-iter", type=int, default=50)
ap.add_argument("--skip-speed", action="store_true")
ap.add_argument("--skip-compression", action="store_true")
a = ap.parse_args()

with np.load(os.path.join(REPO, "tests", "golden", "ref_features.npz")) as z:
    pos_c, neg_c = z["pos_counts"].astype(np.int64), z["neg_counts"].astype(np.int64)
ctx = _lib.get_context()
out = {"workload": "mixture", "reference_rows": [len(pos_c), len(neg_c)], "block_rows": int(ctx.lib.phk_mix_block_rows())}


def speed():
    n, L, k, D = a.contigs, a.length, 4, 256
    T = n * L
    packed = device.DeviceArray(ctx, device.packed_words(T), np.uint32)
    off = device.DeviceArray(ctx, n + 1, np.uint64)
    counts = device.DeviceArray(ctx, (n, D), np.uint32)
    device.synth_packed(ctx, 0, 0, n, L, packed, off)
    device.count(ctx, packed, None, T, off, n, k, counts)
    host_counts = counts.to_host()
    batch = _lib.Batch.from_counts(ctx, host_counts.astype(np.int64))
    res = {"contigs": n, "length": L, "per_K": {}}
    rows = min(a.numpy_rows, n)
    for K in a.components:
        start = np.random.RandomState(K).choice(n, K, replace=False)
        logp, w = likelihood.log_table(host_counts[start], 0.5), np.full(K, 1.0 / K)
        table = _lib.MixtureTable(ctx, logp, np.log(w))
        times = []
        for i in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            got = batch.mixture_expect(table)
            if i >= a.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        ctx.profile_reset()
        ctx.profile_enable(True)
        batch.mixture_expect(table)
        prof = {name: v[0] for name, v in ctx.profile().items()}
        ctx.profile_enable(False)
        table.close()
        fits = {}
        for iters in (2, 6):
            t0 = time.perf_counter()
            m = mixture.fit(batch, K, init=start, max_iter=iters, tol=0.0)
            fits[iters] = (time.perf_counter() - t0) * 1e3
            assert m.n_iter == iters
        q = host_counts[:rows]
        t0 = time.perf_counter()
        c = q.astype(np.float64)
        S = c @ logp.T + np.log(w)[None, :]
        mx = S.max(axis=1)
        l = mx + np.log(np.exp(S - mx[:, None]).sum(axis=1))
        r = np.exp(S - l[:, None])
        Tn, Nn, Ln = r.T @ c, r.sum(axis=0), l.sum()
        numpy_ms = (time.perf_counter() - t0) * 1e3
        flop = 2.0 * n * K * D
        res["per_K"][str(K)] = {
            "estep_ms_per_call": float(np.median(times)), "estep_ms_calls": times,
            "fit_ms_per_iteration": (fits[6] - fits[2]) / 4.0, "fit_ms": fits,
            "per_kernel_ms": prof, "product_tflop": flop / 1e12,
            "resp_kernel_tflops": flop / prof.get("phk_mix_resp_kernel", float("nan")) / 1e9,
            "expect_kernel_tflops": flop / prof.get("phk_mix_expect_kernel", float("nan")) / 1e9,
            "numpy_rows": rows, "numpy_ms": numpy_ms, "numpy_ms_scaled_to_batch": numpy_ms * n / rows,
            "L": got[2], "smallest_Nk": float(got[1].min())}
    log_pos, log_neg = likelihood.log_table(pos_c), likelihood.log_table(neg_c)
    lik = _lib.LikelihoodTable(ctx, log_pos, log_neg)
    times = []
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        batch.likelihood(lik)
        if i >= a.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    res["likelihood_ms_per_call"] = float(np.median(times))
    res["likelihood_product_tflop"] = 2.0 * n * (len(pos_c) + len(neg_c)) * D / 1e12
    lik.close()
    batch.close()
    out["speed"] = res


def compression():
    plan = cross_validate.FoldPlan(len(pos_c), len(neg_c), a.folds, 0)
    rng = np.random.RandomState(0)
    queries = {"full": (pos_c, neg_c)}
    queries.update({str(n): (likelihood.thin(pos_c, n, rng), likelihood.thin(neg_c, n, rng)) for n in a.lengths})
    table = {"likelihood": {}}
    for key, qs in queries.items():
        auc, acc = likelihood.evaluate(*likelihood.cross_validate(pos_c, neg_c, a.folds, 0, _queries=None if key == "full" else qs))
        table["likelihood"][key] = {"auc": float(auc), "accuracy": float(acc)}
    fit_stats = {}
    for K in a.fit_components:
        got = {key: (np.zeros(len(pos_c)), np.zeros(len(neg_c))) for key in queries}
        iters, dead, t0 = [], 0, time.perf_counter()
        for fold in range(plan.folds):
            out_p, out_n = plan.held_out(fold)
            mp = mixture.fit(pos_c[~out_p], K, seed=0, max_iter=a.max_iter)
            mn = mixture.fit(neg_c[~out_n], K, seed=0, max_iter=a.max_iter)
            iters += [mp.n_iter, mn.n_iter]
            dead += int(mp.dead.sum() + mn.dead.sum())
            for key, (qp, qn) in queries.items():
                got[key][0][out_p] = mixture.score(qp[out_p], mp, mn)
                got[key][1][out_n] = mixture.score(qn[out_n], mp, mn)
        fit_stats[str(K)] = {"seconds": time.perf_counter() - t0, "mean_iterations": float(np.mean(iters)),
                             "fits_at_max_iter": int(np.sum(np.array(iters) >= a.max_iter)), "dead_components": dead}
        table["K=%d" % K] = {}
        for key in queries:
            auc, acc = likelihood.evaluate(*got[key])
            table["K=%d" % K][key] = {"auc": float(auc), "accuracy": float(acc)}
    out["compression"] = {"folds": a.folds, "seed": 0, "max_iter": a.max_iter, "table": table, "fits": fit_stats}


if not a.skip_speed:
    speed()
if not a.skip_compression:
    compression()
print(json.dumps(out))
