#!/usr/bin/env python3
"""S-state chain measurements, one JSON line.

chain    For three shapes -- ``--records`` records of 20 windows, one record of 10^4 windows (a 5 Mb genome at 500-base
         windows), one record of ``--long`` windows -- and S = 2, 4, 8 at D = 256: phk_chain_set (the emissions), one E-step
         (phk_chain_expect) and one decode (phk_chain_decode), host clock around calls that end with their results on the
         host, median after warm-up; the kernels' event times from one profiled call of each.  The rows are resident before
         the clock starts (one upload per chain, reported once).  Count rows: uniform 0..3 per column (about 384 k-mers a
         row), default_rng(0); profiles: Dirichlet rows; the chain of compose.start_chain.
         Baseline in the same process: the E-step restated in float64 NumPy (emissions by matmul, probability domain,
         renormalised per step, vectorised across the records of a call; a single record is a per-step loop), timed on the
         first ``--numpy_rows`` rows of the shape and scaled to the call.
two      For S = 2: a chain made from the emissions (0, x) against segment.decode on the same track x of one record of 10^4
         and of ``--long`` windows.  Only the times are compared.
"""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _lib, compose, segment

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--long", type=int, default=1000000, help="windows of the long record")
ap.add_argument("--records", type=int, default=100000, help="records of the many-records shape")
ap.add_argument("--numpy_rows", type=int, default=200000, help="rows the NumPy statement is timed on")
ap.add_argument("--states", type=int, nargs="*", default=[2, 4, 8])
ap.add_argument("--skip", nargs="*", default=[], choices=["chain", "two"])
a = ap.parse_args()
D = 256
out = {"workload": "compose", "D": D}


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


def numpy_estep(C, logp, A, pi, R, n):
    """One E-step over R records of n windows side by side, float64: (T, Ns, xi, L)."""
    S = len(pi)
    E = (C.astype(np.float64) @ logp.T).reshape(R, n, S)
    M = E.max(axis=2)
    e = np.exp(E - M[:, :, None])
    alpha, c = np.empty((R, n, S)), np.empty((R, n))
    v = pi[None, :] * e[:, 0]
    for t in range(n):
        if t:
            v = (alpha[:, t - 1] @ A) * e[:, t]
        c[:, t] = v.sum(axis=1)
        alpha[:, t] = v / c[:, t, None]
    beta = np.ones((R, S))
    gamma = np.empty((R, n, S))
    gamma[:, n - 1] = alpha[:, n - 1]
    xi = np.zeros((S, S))
    for t in range(n - 1, 0, -1):
        w = e[:, t] * beta / c[:, t, None]
        xi += A * (alpha[:, t - 1].T @ w)
        beta = w @ A.T
        gamma[:, t - 1] = alpha[:, t - 1] * beta
    g = gamma.reshape(R * n, S)
    return g.T @ C.astype(np.float64), g.sum(axis=0), xi, float(np.log(c).sum() + M.sum())


def chain():
    ctx = _lib.get_context()
    rng = np.random.default_rng(0)
    shapes = (("many_records_of_20", a.records, 20), ("one_record_1e4", 1, 10000), ("one_record_long", 1, a.long))
    out["chain"] = {}
    for name, R, n in shapes:
        C = rng.integers(0, 4, (R * n, D), dtype=np.uint8).astype(np.uint32)
        off = np.arange(R + 1, dtype=np.uint64) * np.uint64(n)
        out["chain"][name] = {"records": R, "windows_per_record": n}
        for S in a.states:
            logp = np.log(rng.dirichlet(np.full(D, 20.0), S))
            A, pi = compose.start_chain(S)
            qt, qp = segment.quantise(np.log(A)), segment.quantise(np.log(pi))
            t0 = time.perf_counter()
            ch = _lib.Chain(ctx, C, off, S)
            create_ms = (time.perf_counter() - t0) * 1e3
            try:
                _, set_ms, _ = timed(lambda: ch.set(logp, A, pi, qt, qp, 1.0))
                got, expect_ms, expect_calls = timed(lambda: ch.expect())
                dec, decode_ms, decode_calls = timed(lambda: ch.decode())
                prof_set = profiled(ctx, lambda: ch.set(logp, A, pi, qt, qp, 1.0))
                prof_expect = profiled(ctx, lambda: ch.expect())
                prof_decode = profiled(ctx, lambda: ch.decode())
            finally:
                ch.close()
            rows = min(R * n, max(n, a.numpy_rows // n * n)) if R > 1 else min(n, a.numpy_rows)
            Rn, nn = (rows // n, n) if R > 1 else (1, rows)
            t0 = time.perf_counter()
            ref = numpy_estep(C[:rows], logp, A, pi, Rn, nn)
            numpy_ms = (time.perf_counter() - t0) * 1e3
            row = {"create_ms": create_ms, "set_ms_per_call": set_ms, "expect_ms_per_call": expect_ms,
                   "expect_ms_calls": expect_calls, "decode_ms_per_call": decode_ms, "decode_ms_calls": decode_calls,
                   "kernel_ms_set": prof_set, "kernel_ms_expect": prof_expect, "kernel_ms_decode": prof_decode,
                   "windows_per_second_expect": R * n / (expect_ms * 1e-3), "windows_per_second_decode": R * n / (decode_ms * 1e-3),
                   "numpy_rows_timed": rows, "numpy_ms": numpy_ms, "numpy_ms_scaled_to_the_call": numpy_ms * R * n / rows}
            if rows == R * n:
                row["max_rel_T_diff_numpy"] = float(np.abs(got[0] - ref[0]).max() / np.abs(ref[0]).max())
                row["log_evidence_diff_numpy"] = float(abs(got[4] - ref[3]))
            out["chain"][name]["S%d" % S] = row


def two():
    ctx = _lib.get_context()
    rng = np.random.default_rng(1)
    p_enter, p_leave = 0.05, 0.1
    trans, init, qt, qp = segment.parameters(p_enter, p_leave)
    out["two"] = {}
    for name, n in (("one_record_1e4", 10000), ("one_record_long", a.long)):
        sign = np.repeat(rng.choice([-2.0, 2.0], size=n // 37 + 1), 37)[:n]
        x = 3.0 * rng.standard_normal(n) + sign
        off = np.array([0, n], dtype=np.uint64)
        E = np.stack((np.zeros(n), x), axis=1)

        def chain_decode():
            ch = _lib.Chain(ctx, E, off, 2, emissions=True)
            try:
                ch.set(None, trans.reshape(2, 2), init, qt.reshape(2, 2), qp, 1.0)
                return ch.decode()
            finally:
                ch.close()

        seg_ms, chain_ms = [], []
        for i in range(a.warmup + a.steps):          # alternated: both see the same clocks
            t0 = time.perf_counter()
            d = segment.decode(x, off, p_enter, p_leave)
            t1 = time.perf_counter()
            c = chain_decode()
            t2 = time.perf_counter()
            if i >= a.warmup:
                seg_ms.append((t1 - t0) * 1e3)
                chain_ms.append((t2 - t1) * 1e3)
        out["two"][name] = {"windows": n, "segment_decode_ms": float(np.median(seg_ms)), "chain_decode_ms": float(np.median(chain_ms)),
                            "segment_ms_calls": seg_ms, "chain_ms_calls": chain_ms, "states_differ": int((d.state != c[0]).sum())}


for name, fn in (("chain", chain), ("two", two)):
    if name not in a.skip:
        fn()
print(json.dumps(out))
