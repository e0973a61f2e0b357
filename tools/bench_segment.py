#!/usr/bin/env python3
"""Track segmentation measurements, one JSON line.

decode  segment.decode alone (host clock around calls that end with the four outputs on the host, median after warm-up;
        the kernels' event times from one profiled call) for three shapes: one record of 10^4 windows, one of 2 * 10^7,
        10^6 records of 20.  Evidence: tests' kind, normal of scale 3 with biased runs, default_rng(0).
        Baseline: the forward-backward restated in float64 NumPy, probability domain, renormalised per step, vectorised
        across the records of a call where there are several; a single record is a per-step Python loop, timed on its first
        ``--numpy_steps`` windows and scaled to the record (the parent commit has no decode to compare with).  The baseline
        computes posterior and log_odds only, no Viterbi path.
e2e     python -m phamers_amd.windows on a random ``--genome`` base sequence (one record, default_rng(1)), -m likelihood
        -w 500 -s 500 against the golden reference counts, with and without --segment: host clock around main().
"""
import argparse, json, os, sys, tempfile, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _lib, fileIO, segment, windows

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--long", type=int, default=20000000, help="windows of the long record")
ap.add_argument("--records", type=int, default=1000000, help="records of the many-records shape")
ap.add_argument("--numpy_steps", type=int, default=200000, help="windows the per-step NumPy loop is timed on")
ap.add_argument("--genome", type=int, default=5000000)
ap.add_argument("--skip", nargs="*", default=[], choices=["decode", "e2e"])
a = ap.parse_args()
A, B = 0.05, 0.1
out = {"workload": "segment", "p_enter": A, "p_leave": B}


def evidence(rng, n, run=37):
    sign = np.repeat(rng.choice([-2.0, 2.0], size=n // run + 1), run)[:n]
    return 3.0 * rng.standard_normal(n) + sign


def numpy_forward_backward(x, trans, init):
    """x (R, n): R records of n windows side by side -> (posterior (R, n), log_odds (R,)), float64."""
    R, n = x.shape
    e1 = np.exp(-np.abs(x))
    em = np.stack((np.where(x > 0, e1, 1.0), np.where(x > 0, 1.0, e1)), axis=2)          # (R, n, 2), scaled by exp(-max(x, 0))
    Am = np.asarray(trans).reshape(2, 2)
    alpha, beta = np.empty((R, n, 2)), np.empty((R, n, 2))
    logz = np.maximum(x, 0.0).sum(axis=1)
    v = init[None, :] * em[:, 0]
    for t in range(n):
        if t:
            v = (alpha[:, t - 1] @ Am) * em[:, t]
        s = v.sum(axis=1, keepdims=True)
        alpha[:, t] = v / s
        logz += np.log(s[:, 0])
    beta[:, n - 1] = 1.0
    for t in range(n - 1, 0, -1):
        v = (em[:, t] * beta[:, t]) @ Am.T
        beta[:, t - 1] = v / v.sum(axis=1, keepdims=True)
    p = alpha * beta
    return p[:, :, 1] / p.sum(axis=2), logz


def timed(fn):
    times = []
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        r = fn()
        if i >= a.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return r, float(np.median(times)), times


def decode():
    ctx = _lib.get_context()
    trans, init, _, _ = segment.parameters(A, B)
    rng = np.random.default_rng(0)
    shapes = (("one_record_1e4", 1, 10000), ("one_record_long", 1, a.long), ("many_records_of_20", a.records, 20))
    out["decode"] = {}
    for name, R, n in shapes:
        x = evidence(rng, R * n)
        off = (np.arange(R + 1, dtype=np.uint64) * np.uint64(n))
        d, ms, calls = timed(lambda: segment.decode(x, off, A, B))
        ctx.profile_reset()
        ctx.profile_enable(True)
        segment.decode(x, off, A, B)
        prof = {k: v[0] for k, v in ctx.profile().items()}
        ctx.profile_enable(False)
        m = n if R > 1 else min(n, a.numpy_steps)
        t0 = time.perf_counter()
        post, lo = numpy_forward_backward(x.reshape(R, n)[:, :m], trans, init)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        row = {"records": R, "windows_per_record": n, "decode_ms_per_call": ms, "decode_ms_calls": calls,
               "kernel_ms": prof, "kernels_ms_total": float(sum(prof.values())),
               "windows_per_second": R * n / (ms * 1e-3), "phage_windows": int(d.state.sum()),
               "numpy_windows_timed": R * m, "numpy_ms": numpy_ms, "numpy_ms_scaled_to_the_call": numpy_ms * n / m}
        if m == n:      # (the whole call restated: how far the device is from float64 NumPy)
            row["max_posterior_diff_numpy"] = float(np.abs(post.ravel() - d.posterior).max())
            row["max_log_odds_diff_numpy"] = float(np.abs(lo - d.log_odds).max())
        out["decode"][name] = row


def e2e():
    with np.load(os.path.join(REPO, "tests", "golden", "ref_features.npz")) as z:
        pos, neg = z["pos_counts"].astype(np.int64), z["neg_counts"].astype(np.int64)
    rng = np.random.default_rng(1)
    seq = np.frombuffer(b"ATGC", dtype=np.uint8)[rng.integers(0, 4, a.genome)].tobytes().decode()
    with tempfile.TemporaryDirectory() as tmp:
        fasta = os.path.join(tmp, "genome.fasta")
        with open(fasta, "w") as f:
            f.write(">genome\n" + "\n".join(seq[i:i + 80] for i in range(0, len(seq), 80)) + "\n")
        fileIO.save_counts(pos, ["p%d" % i for i in range(len(pos))], os.path.join(tmp, "pos.csv"))
        fileIO.save_counts(neg, ["n%d" % i for i in range(len(neg))], os.path.join(tmp, "neg.csv"))
        base = ["-in", fasta, "-out", os.path.join(tmp, "out"), "-pf", os.path.join(tmp, "pos.csv"), "-nf",
                os.path.join(tmp, "neg.csv"), "-m", "likelihood", "-w", "500", "-s", "500"]
        times = {"plain": [], "segment": []}
        for i in range(a.warmup + a.steps):           # alternated: both see the same clocks
            for name, argv in (("plain", base), ("segment", base + ["--segment"])):
                t0 = time.perf_counter()
                track, _ = windows.main(argv)
                if i >= a.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        out["e2e"] = {"bases": a.genome, "windows": len(track), "plain_ms_per_run": float(np.median(times["plain"])),
                      "segment_ms_per_run": float(np.median(times["segment"])), "plain_ms_runs": times["plain"],
                      "segment_ms_runs": times["segment"]}


for name, fn in (("decode", decode), ("e2e", e2e)):
    if name not in a.skip:
        fn()
print(json.dumps(out))
