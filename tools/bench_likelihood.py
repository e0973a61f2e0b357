#!/usr/bin/env python3
"""Likelihood scoring measurements, one JSON line.

speed   2^20 resident synthetic 5 kb contigs (phk_synth_packed_dev, counted once on the device) against the full PhaMers
        4-mer reference (2 255 + 2 418 count rows): ms per scoring call of Batch.likelihood, alternated in the same process
        with the density method on the same resident counts (the yardstick: the same 2 N M D float64 product), host clock
        around calls that end in a device synchronise, median after warm-up; the kernels' event times; and the NumPy
        float64 statement on the host for ``--numpy-rows`` of the contigs, scaled to the batch.
tables  (b) the 20-fold seed-0 cross validation of the reference rows: AUC and accuracy at threshold 0, raw and per k-mer;
        (c) the same folds with every held-out row thinned to n k-mers (likelihood.thin), for likelihood, density at
        bandwidths 0.005 / 0.005 and combo at the defaults, each on the same thinned rows.
"""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _lib, cross_validate, device, kmer, likelihood

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=1 << 20)
ap.add_argument("--length", type=int, default=5000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--numpy-rows", type=int, default=4096)
ap.add_argument("--folds", type=int, default=20)
ap.add_argument("--lengths", type=int, nargs="*", default=[200, 500, 1000, 2000, 5000])
ap.add_argument("--skip-speed", action="store_true")
ap.add_argument("--skip-tables", action="store_true")
a = ap.parse_args()

with np.load(os.path.join(REPO, "tests", "golden", "ref_features.npz")) as z:
    pos_c, neg_c = z["pos_counts"].astype(np.int64), z["neg_counts"].astype(np.int64)
ctx = _lib.get_context()
out = {"workload": "likelihood", "reference_rows": [len(pos_c), len(neg_c)]}


def speed():
    n, L, k, D = a.contigs, a.length, 4, 256
    M, T = len(pos_c) + len(neg_c), a.contigs * a.length
    packed = device.DeviceArray(ctx, device.packed_words(T), np.uint32)
    off = device.DeviceArray(ctx, n + 1, np.uint64)
    counts = device.DeviceArray(ctx, (n, D), np.uint32)
    scores = device.DeviceArray(ctx, n, np.float64)
    status = device.DeviceArray.from_host(ctx, np.zeros(1, np.uint32))
    device.synth_packed(ctx, 0, 0, n, L, packed, off)
    device.count(ctx, packed, None, T, off, n, k, counts)
    host_counts = counts.to_host()
    batch = _lib.Batch.from_counts(ctx, host_counts.astype(np.int64))
    log_pos, log_neg = likelihood.log_table(pos_c), likelihood.log_table(neg_c)
    table = _lib.LikelihoodTable(ctx, log_pos, log_neg)
    model = _lib.Model(ctx, kmer.normalize_counts(pos_c), kmer.normalize_counts(neg_c), k_neighbors=3)
    last = {}

    def lik():
        last["s"] = batch.likelihood(table)      # (synchronous: the three result vectors come back)

    def density():
        device.score_counts(ctx, model, counts, n, "density", scores, status)
        ctx.sync()
    times = {"likelihood": [], "density": []}
    for i in range(a.warmup + a.steps):           # alternated: both see the same clocks and the same neighbours
        for name, fn in (("likelihood", lik), ("density", density)):
            t0 = time.perf_counter()
            fn()
            if i >= a.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    ctx.profile_reset()
    ctx.profile_enable(True)
    lik()
    density()
    prof = {name: v[0] for name, v in ctx.profile().items()}
    ctx.profile_enable(False)
    rows = min(a.numpy_rows, n)
    q = host_counts[:rows].astype(np.float64)
    t0 = time.perf_counter()
    want = []
    for table_c in (log_pos, log_neg):
        S = q @ table_c.T
        m = S.max(axis=1)
        want.append(m + np.log(np.exp(S - m[:, None]).sum(axis=1)) - np.log(len(table_c)))
    numpy_ms = (time.perf_counter() - t0) * 1e3
    want = want[0] - want[1]
    gram = 2.0 * n * M * D
    ms_l, ms_d = float(np.median(times["likelihood"])), float(np.median(times["density"]))
    s = last["s"]
    out["speed"] = {
        "contigs": n, "length": L, "gram_tflop": gram / 1e12,
        "likelihood_ms_per_call": ms_l, "likelihood_ms_calls": times["likelihood"],
        "density_ms_per_call": ms_d, "density_ms_calls": times["density"], "likelihood_over_density": ms_l / ms_d,
        "likelihood_gram_tflops": gram / ms_l / 1e9, "density_gram_tflops": gram / ms_d / 1e9,
        "lik_partial_kernel_ms": prof.get("phk_lik_partial_kernel"), "kde_partial_kernel_ms": prof.get("phk_kde_partial_kernel"),
        "lik_partial_kernel_tflops": gram / prof.get("phk_lik_partial_kernel", float("nan")) / 1e9,
        "kde_partial_kernel_tflops": gram / prof.get("phk_kde_partial_kernel", float("nan")) / 1e9,
        "per_kernel_ms": prof, "numpy_rows": rows, "numpy_ms": numpy_ms, "numpy_ms_scaled_to_batch": numpy_ms * n / rows,
        "numpy_max_abs_diff": float(np.max(np.abs(s[:rows] - want))),
        "score_mean": float(np.mean(s)), "score_min": float(np.min(s)), "score_max": float(np.max(s)),
        "fraction_scored_phage": float(np.mean(s >= 0))}
    batch.close()
    table.close()
    model.close()


def tables():
    P, Nm = kmer.normalize_counts(pos_c), kmer.normalize_counts(neg_c)
    plan = cross_validate.FoldPlan(len(pos_c), len(neg_c), a.folds, 0)
    rng = np.random.RandomState(0)
    thinned = {n: (likelihood.thin(pos_c, n, rng), likelihood.thin(neg_c, n, rng)) for n in a.lengths}
    rows = {}
    t0 = time.perf_counter()
    for per_kmer in (False, True):
        name = "likelihood_per_kmer" if per_kmer else "likelihood"
        rows[name] = {"full": likelihood.evaluate(*likelihood.cross_validate(pos_c, neg_c, a.folds, 0, per_kmer=per_kmer))}
        for n, qs in thinned.items():
            rows[name][str(n)] = likelihood.evaluate(
                *likelihood.cross_validate(pos_c, neg_c, a.folds, 0, per_kmer=per_kmer, _queries=qs))
    out["likelihood_tables_seconds"] = time.perf_counter() - t0
    # density and combo: one resident model, a fold = a column mask (+ its centroids), as cross_validator runs them; the
    # fold's model scores the held-out rows as they are and thinned to every length
    queries = {"full": (P, Nm)}
    queries.update({str(n): (kmer.normalize_counts(qs[0].astype(np.int64)), kmer.normalize_counts(qs[1].astype(np.int64)))
                    for n, qs in thinned.items()})
    v = cross_validate.cross_validator()
    for method in ("density", "combo"):
        got = {key: (np.zeros(len(P)), np.zeros(len(Nm))) for key in queries}
        model = None
        for fold in range(plan.folds):
            out_p, out_n = plan.held_out(fold)
            cents = (v._fold_centroids(P[~out_p]), v._fold_centroids(Nm[~out_n])) if method == "combo" else (None, None)
            if model is not None and method == "combo":
                model.close()
                model = None
            if model is None:
                model = _lib.Model(ctx, P, Nm, cents[0], cents[1], k_neighbors=3)
                if method == "density":
                    model.set_bandwidths(0.005, 0.005)
            model.set_column_mask(np.concatenate((out_p, out_n)))
            for key, (qp, qn) in queries.items():
                s = model.score(np.vstack((qp[out_p], qn[out_n])), method)
                n_p = int(out_p.sum())
                got[key][0][out_p], got[key][1][out_n] = s[:n_p], s[n_p:]
        model.close()
        rows[method] = {key: likelihood.evaluate(*got[key]) for key in got}
    out["tables"] = {m: {k: {"auc": float(v2[0]), "accuracy": float(v2[1])} for k, v2 in r.items()} for m, r in rows.items()}
    out["folds"], out["seed"] = a.folds, 0


if not a.skip_speed:
    speed()
if not a.skip_tables:
    tables()
print(json.dumps(out))
