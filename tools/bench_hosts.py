#!/usr/bin/env python3
"""Likelihood-ranked lookup measurements, one JSON line.

iid     (a) retrieval on independent draws: the 2 418 bacterial count rows, each thinned to n k-mers (likelihood.thin,
        RandomState(0)), ranked against all 2 418 rows (top 5) with the multinomial table, the Markov table and Euclidean
        distance on frequencies (learning.kneighbors): the share of queries whose own genome comes back first / among the
        first five.  The device rankings are checked against the NumPy float64 statement: indices equal, S within the bound.
chain   (b) the same table for sequences sampled from each genome's own order-3 chain (the transition probabilities of its
        4-mer counts, pseudocount 0.5; first 3-mer from the genome's 3-mer frequencies; default_rng(0)) and counted with
        kmer.count.  Independent draws are the multinomial model's own data and chain samples the Markov model's: the two
        tables belong side by side.
speed   (c) 2^20 resident synthetic 5 kb contigs ranked (top 5, Markov table) against the 2 418 hosts by Batch.hosts,
        alternated in the same process with Batch.likelihood on a one-class table of the same rows; host clock around calls
        that end with the results on the host, median after warm-up; the kernels' event times.
null    (d) hosts.fit_null of the 2 255 phage rows against the 2 418 hosts, per call.
"""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _lib, device, hosts, kmer, learning, likelihood

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=1 << 20)
ap.add_argument("--length", type=int, default=5000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--lengths", type=int, nargs="*", default=[500, 2000, 5000, 20000])
ap.add_argument("--rows", type=int, default=0, help="use only the first ROWS genomes (0 = all; for a rehearsal)")
ap.add_argument("--skip", nargs="*", default=[], choices=["iid", "chain", "speed", "null"])
a = ap.parse_args()

with np.load(os.path.join(REPO, "tests", "golden", "ref_features.npz")) as z:
    pos_c, neg_c = z["pos_counts"].astype(np.int64), z["neg_counts"].astype(np.int64)
if a.rows:
    pos_c, neg_c = pos_c[:a.rows], neg_c[:a.rows]
M = len(neg_c)
U = 2.0 ** -53
out = {"workload": "hosts", "hosts": M, "null_rows": len(pos_c)}


def shares(idx):
    own = np.arange(len(idx))[:, None]
    return [float((idx[:, 0:1] == own).mean()), float((idx == own).any(axis=1).mean())]


def retrieval(queries):
    """{method: [top-1, top-5]} of count rows queries[i] drawn from genome i, and the check against NumPy."""
    row, X = {}, kmer.normalize_counts(neg_c)
    for model in hosts.MODELS:
        r = hosts.rank(queries, neg_c, top=5, model=model)
        row[model] = shares(r.indices)
        L = hosts._table(neg_c, model, 0.5)
        c = queries.astype(np.float64)
        S = c @ L.T
        order = np.lexsort((np.broadcast_to(np.arange(M), S.shape), -S), axis=1)[:, :5]
        e = (c.shape[1] + 2) * U * (c @ np.abs(L).T).max(axis=1)
        err = np.abs(r.log_likelihood - np.take_along_axis(S, r.indices, axis=1))
        row[model + "_numpy"] = shares(order)
        row[model + "_indices_equal_numpy"] = float((order == r.indices).all(axis=1).mean())
        row[model + "_max_S_err_over_2e"] = float((err / (2.0 * e[:, None])).max())
    q = kmer.normalize_counts(queries.astype(np.int64))
    row["euclidean"] = shares(learning.kneighbors(q, X, k=5)[1])
    return row


def iid():
    rng = np.random.RandomState(0)
    out["iid"] = {str(n): retrieval(likelihood.thin(neg_c, n, rng)) for n in a.lengths}


def chain_sequences(n_max):
    """One sequence of n_max + 3 bases per genome from its own order-3 chain, as codes in kmer.py's digit order."""
    rng = np.random.default_rng(0)
    x = neg_c.astype(np.float64).reshape(M, 64, 4)
    cum = np.cumsum((x + 0.5) / (x.sum(axis=2, keepdims=True) + 2.0), axis=2)[:, :, :3]
    start = np.cumsum(x.sum(axis=2) / x.sum(axis=(1, 2))[:, None], axis=1)[:, :63]
    state = (rng.random(M)[:, None] > start).sum(axis=1)
    codes = np.empty((M, n_max + 3), dtype=np.uint8)
    codes[:, 0], codes[:, 1], codes[:, 2] = state // 16, (state // 4) % 4, state % 4
    rows = np.arange(M)
    for t in range(3, n_max + 3):
        b = (rng.random(M)[:, None] > cum[rows, state]).sum(axis=1)
        codes[:, t] = b
        state = (state * 4 + b) % 64
    return codes


def chain():
    codes = chain_sequences(max(a.lengths))
    letters = np.frombuffer(kmer.DNA.encode() if isinstance(kmer.DNA, str) else bytes(kmer.DNA), dtype=np.uint8)
    out["chain"] = {}
    for n in a.lengths:
        seqs = [letters[row].tobytes().decode() for row in codes[:, :n + 3]]
        counts = np.asarray(kmer.count(seqs, 4))
        assert counts.shape == (M, 256) and (counts.sum(axis=1) == n).all()
        out["chain"][str(n)] = retrieval(counts)


def speed():
    n, L, k, D = a.contigs, a.length, 4, 256
    ctx = _lib.get_context()
    T = n * L
    packed = device.DeviceArray(ctx, device.packed_words(T), np.uint32)
    off = device.DeviceArray(ctx, n + 1, np.uint64)
    counts = device.DeviceArray(ctx, (n, D), np.uint32)
    device.synth_packed(ctx, 0, 0, n, L, packed, off)
    device.count(ctx, packed, None, T, off, n, k, counts)
    host_counts = counts.to_host()
    batch = _lib.Batch.from_counts(ctx, host_counts.astype(np.int64))
    table = _lib.HostTable(ctx, hosts.markov_log_table(neg_c))
    lik = _lib.LikelihoodTable(ctx, likelihood.log_table(neg_c))
    last = {}

    def rank():
        last["r"] = batch.hosts(table, 5)            # (synchronous: indices and S come back)

    def score():
        last["s"] = batch.likelihood(lik)
    times = {"rank": [], "likelihood": []}
    for i in range(a.warmup + a.steps):               # alternated: both see the same clocks and the same neighbours
        for name, fn in (("rank", rank), ("likelihood", score)):
            t0 = time.perf_counter()
            fn()
            if i >= a.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    ctx.profile_reset()
    ctx.profile_enable(True)
    rank()
    score()
    prof = {name: v[0] for name, v in ctx.profile().items()}
    ctx.profile_enable(False)
    rows = min(4096, n)
    S = host_counts[:rows].astype(np.float64) @ hosts.markov_log_table(neg_c).T
    order = np.lexsort((np.broadcast_to(np.arange(M), S.shape), -S), axis=1)[:, :5]
    gram = 2.0 * n * M * D
    ms_r, ms_l = float(np.median(times["rank"])), float(np.median(times["likelihood"]))
    out["speed"] = {
        "contigs": n, "length": L, "top": 5, "gram_tflop": gram / 1e12,
        "rank_ms_per_call": ms_r, "rank_ms_calls": times["rank"], "likelihood_ms_per_call": ms_l,
        "likelihood_ms_calls": times["likelihood"], "rank_over_likelihood": ms_r / ms_l,
        "rank_kernel_ms": prof.get("phk_host_rank_kernel"), "merge_kernel_ms": prof.get("phk_host_merge_kernel"),
        "lik_partial_kernel_ms": prof.get("phk_lik_partial_kernel"),
        "rank_kernel_tflops": gram / prof.get("phk_host_rank_kernel", float("nan")) / 1e9,
        "lik_partial_kernel_tflops": gram / prof.get("phk_lik_partial_kernel", float("nan")) / 1e9,
        "per_kernel_ms": prof, "result_bytes_to_host": int(n * 5 * 12),
        "numpy_rows": rows, "numpy_indices_equal": float((order == last["r"][0][:rows]).all(axis=1).mean())}
    batch.close()
    table.close()
    lik.close()


def null():
    times = []
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        mu, sigma = hosts.fit_null(pos_c, neg_c, model='markov')
        if i >= a.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    ctx = _lib.get_context()
    table = _lib.HostTable(ctx, hosts.markov_log_table(neg_c))
    ctx.profile_reset()
    ctx.profile_enable(True)
    table.null_fit(pos_c.astype(np.uint32))
    prof = {name: v[0] for name, v in ctx.profile().items()}
    ctx.profile_enable(False)
    table.close()
    ell = (pos_c @ hosts.markov_log_table(neg_c).T) / pos_c.sum(axis=1)[:, None]
    out["null"] = {"rows": len(pos_c), "hosts": M, "fit_ms_per_call": float(np.median(times)), "fit_ms_calls": times,
                   "per_kernel_ms": prof, "mu_range": [float(mu.min()), float(mu.max())],
                   "sigma_range": [float(sigma.min()), float(sigma.max())],
                   "mu_max_abs_diff_numpy": float(np.abs(mu - ell.mean(axis=0)).max()),
                   "sigma_max_abs_diff_numpy": float(np.abs(sigma - ell.std(axis=0, ddof=1)).max())}


for name, fn in (("iid", iid), ("chain", chain), ("speed", speed), ("null", null)):
    if name not in a.skip:
        fn()
print(json.dumps(out))
