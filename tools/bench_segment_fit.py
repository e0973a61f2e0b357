#!/usr/bin/env python3
"""Segmentation fit measurements, one JSON line.

Three workloads, evidence of tools/bench_segment.py's kind (normal of scale 3 with biased runs, default_rng(0)):
10^6 records of 20 windows, one record of 2 * 10^7 windows, one track of 10^4 windows.

fit     time per EM iteration: ``segment.fit`` with a fixed start and tol = 0 is timed at two iteration counts (host clock,
        median after warm-up) and the difference divided by the E-steps between them, so the one upload of a fit drops
        out; the whole fit's time at the smaller count is reported beside it.  The kernels' event times come from one
        profiled ``segment.expected_counts`` call (one E-step).
decode  ``segment.decode`` on the same data, host clock and kernel event times: what an iteration is compared with.  Run
        with ``--only decode`` under another build of the library to time that build's decode in the same visit.
numpy   the E-step restated in float64 NumPy (probability domain, renormalised per step, vectorised across the records of
        a call; a single record is a per-step Python loop, timed on its first ``--numpy_steps`` windows and scaled).
"""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _lib, segment

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--long", type=int, default=20000000, help="windows of the long record")
ap.add_argument("--records", type=int, default=1000000, help="records of the many-records shape")
ap.add_argument("--iterations", type=int, nargs=2, default=[2, 10], help="the two M-step counts a fit is timed at")
ap.add_argument("--numpy_steps", type=int, default=100000, help="windows the per-step NumPy loop is timed on")
ap.add_argument("--only", nargs="*", default=["fit", "decode", "numpy"], choices=["fit", "decode", "numpy"])
a = ap.parse_args()
A, B, START = 0.05, 0.1, 0.3
out = {"workload": "segment_fit", "p_enter": A, "p_leave": B, "p_start": START,
       "library": "PHAMERS_AB_LIB" if os.environ.get("PHAMERS_AB_LIB") else "in-tree"}


def evidence(rng, n, run=37):
    sign = np.repeat(rng.choice([-2.0, 2.0], size=n // run + 1), run)[:n]
    return 3.0 * rng.standard_normal(n) + sign


def numpy_e_step(x, trans, init):
    """x (R, n) -> (totals (6,), log evidence), float64."""
    R, n = x.shape
    e1 = np.exp(-np.abs(x))
    em = np.stack((np.where(x > 0, e1, 1.0), np.where(x > 0, 1.0, e1)), axis=2)
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
    g = alpha[:, 0] * beta[:, 0]
    g /= g.sum(axis=1, keepdims=True)
    xi = np.zeros((R, 4))
    for t in range(1, n):
        w = alpha[:, t - 1, :, None] * Am[None] * (em[:, t] * beta[:, t])[:, None, :]
        xi += (w / w.sum(axis=(1, 2), keepdims=True)).reshape(R, 4)
    return np.concatenate((xi.sum(axis=0), g.sum(axis=0))), float(logz.sum())


def timed(fn):
    times = []
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        r = fn()
        if i >= a.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return r, float(np.median(times)), times


def profiled(ctx, fn):
    ctx.profile_reset()
    ctx.profile_enable(True)
    fn()
    prof = {k: v[0] for k, v in ctx.profile().items()}
    ctx.profile_enable(False)
    return prof


ctx = _lib.get_context()
trans, init, _, _ = segment.parameters(A, B, START)
rng = np.random.default_rng(0)
for name, R, n in (("many_records_of_20", a.records, 20), ("one_record_long", 1, a.long), ("one_track_1e4", 1, 10000)):
    x = evidence(rng, R * n)
    off = np.arange(R + 1, dtype=np.uint64) * np.uint64(n)
    row = out[name] = {"records": R, "windows_per_record": n}
    if "fit" in a.only:
        k1, k2 = a.iterations
        f1, ms1, calls1 = timed(lambda: segment.fit(x, off, A, B, p_start=START, max_iter=k1, tol=0.0))
        f2, ms2, calls2 = timed(lambda: segment.fit(x, off, A, B, p_start=START, max_iter=k2, tol=0.0))
        steps = f2.n_iter - f1.n_iter
        prof = profiled(ctx, lambda: segment.expected_counts(x, off, A, B, p_start=START))
        e, ems, ecalls = timed(lambda: segment.expected_counts(x, off, A, B, p_start=START))
        row["fit"] = {"m_steps": [f1.n_iter, f2.n_iter], "fit_ms": [ms1, ms2], "fit_ms_calls": [calls1, calls2],
                      "ms_per_iteration": (ms2 - ms1) / steps if steps > 0 else None,
                      "kernel_ms": prof, "kernels_ms_total": float(sum(prof.values())),
                      "expected_counts_ms_per_call": ems, "expected_counts_ms_calls": ecalls,
                      "p_enter": f2.p_enter, "p_leave": f2.p_leave, "log_evidence": [float(v) for v in f2.trace[:, 9]]}
    if "decode" in a.only:
        d, ms, calls = timed(lambda: segment.decode(x, off, A, B, p_start=START))
        prof = profiled(ctx, lambda: segment.decode(x, off, A, B, p_start=START))
        row["decode"] = {"decode_ms_per_call": ms, "decode_ms_calls": calls, "kernel_ms": prof,
                         "kernels_ms_total": float(sum(prof.values()))}
    if "numpy" in a.only:
        m = n if R > 1 else min(n, a.numpy_steps)
        t0 = time.perf_counter()
        totals, L = numpy_e_step(x.reshape(R, n)[:, :m], trans, init)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        row["numpy"] = {"windows_timed": R * m, "numpy_ms": numpy_ms, "numpy_ms_scaled_to_the_call": numpy_ms * n / m}
        if m == n and "fit" in a.only:
            e = segment.expected_counts(x, off, A, B, p_start=START)
            row["numpy"]["max_relative_totals_diff"] = float(np.max(np.abs(e.totals - totals) / totals))
            row["numpy"]["log_evidence_diff"] = float(abs(e.log_evidence - L))
print(json.dumps(out))
