#!/usr/bin/env python3
"""The tile scan of the S-state chain against the per-record route, one JSON line.

shapes     tools/bench_compose.py's three shapes -- ``--records`` records of 20 windows, one record of 10^4 windows, one record
           of ``--long`` windows -- at D = 256 and S = 2, 4, 8, rows resident, parameters set once: one E-step
           (phk_chain_expect) and one decode (phk_chain_decode) with the route off and on, alternated call by call in one
           process, host clock around calls that end with their results on the host; median, minimum and maximum after
           warm-up, and the kernels' event times from one profiled call of each on either route.  The single records are
           scanned whatever their length (scan_from = 1); the many short records run with ``scan=True``
           (compose.SCAN_FROM), which none of them reaches.  The per-record route in the same run is the yardstick.
           Compared besides the times: states and path scores (must be equal), the largest posterior difference, the
           evidence difference; for the short records every output bit for bit.
threshold  one record of 256, 1 024, 4 096 and 16 384 windows: the E-step with the route off and on, alternated;
           ``scan_from_measured`` = the smallest of these lengths from which the scan is the faster one at every S
           and at every longer length measured.
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
ap.add_argument("--states", type=int, nargs="*", default=[2, 4, 8])
ap.add_argument("--lengths", type=int, nargs="*", default=[256, 1024, 4096, 16384])
ap.add_argument("--skip", nargs="*", default=[], choices=["shapes", "threshold"])
a = ap.parse_args()
D = 256
out = {"workload": "compose_scan", "D": D, "tile": int(_lib.load().phk_chain_tile()), "scan_from_default": compose.SCAN_FROM}


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "calls_ms": ms}


def alternated(ch, scan_from, calls, reps, warmup):
    """{name: {"off": [ms], "on": [ms]}} and the last results of every call on either route."""
    ms = {name: {"off": [], "on": []} for name in calls}
    last = {}
    for i in range(warmup + reps):
        for route, threshold in (("off", 0), ("on", scan_from)):
            ch.set_scan(threshold)
            for name, fn in calls.items():
                t0 = time.perf_counter()
                last[name, route] = fn()
                if i >= warmup:
                    ms[name][route].append((time.perf_counter() - t0) * 1e3)
    return ms, last


def profiled(ctx, fn):
    ctx.profile_reset()
    ctx.profile_enable(True)
    fn()
    prof = {k: v[0] for k, v in ctx.profile().items()}
    ctx.profile_enable(False)
    return prof


def problem(rng, R, n, S):
    C = rng.integers(0, 4, (R * n, D), dtype=np.uint8).astype(np.uint32)
    off = np.arange(R + 1, dtype=np.uint64) * np.uint64(n)
    logp = np.log(rng.dirichlet(np.full(D, 20.0), S))
    A, pi = compose.start_chain(S)
    return C, off, logp, A, pi, segment.quantise(np.log(A)), segment.quantise(np.log(pi))


def shapes():
    ctx = _lib.get_context()
    rng = np.random.default_rng(0)
    out["shapes"] = {}
    for name, R, n in (("many_records_of_20", a.records, 20), ("one_record_1e4", 1, 10000), ("one_record_long", 1, a.long)):
        out["shapes"][name] = {"records": R, "windows_per_record": n}
        scan_from = 1 if R == 1 else compose.SCAN_FROM
        for S in a.states:
            C, off, logp, A, pi, qt, qp = problem(rng, R, n, S)
            ch = _lib.Chain(ctx, C, off, S)
            try:
                ch.set(logp, A, pi, qt, qp, 1.0)
                ms, last = alternated(ch, scan_from, {"expect": lambda: ch.expect(records=True), "decode": ch.decode},
                                      a.steps, a.warmup)
                prof = {}
                for route, threshold in (("off", 0), ("on", scan_from)):
                    ch.set_scan(threshold)
                    prof[route] = {"expect": profiled(ctx, ch.expect), "decode": profiled(ctx, ch.decode)}
            finally:
                ch.close()
            row = {"scan_from": scan_from}
            for call in ("expect", "decode"):
                row[call] = {route: stats(ms[call][route]) for route in ("off", "on")}
                row[call]["off_over_on"] = row[call]["off"]["median_ms"] / row[call]["on"]["median_ms"]
                row[call]["faster_by_more_than_the_spread"] = bool(row[call]["on"]["max_ms"] < row[call]["off"]["min_ms"])
                row[call]["kernel_ms_off"], row[call]["kernel_ms_on"] = prof["off"][call], prof["on"][call]
            e0, e1, d0, d1 = last["expect", "off"], last["expect", "on"], last["decode", "off"], last["decode", "on"]
            row["states_differ"] = int((d0[0] != d1[0]).sum())
            row["path_scores_differ"] = int((d0[3] != d1[3]).sum())
            row["max_posterior_diff"] = float(np.abs(d0[1] - d1[1]).max())
            row["max_rel_T_diff"] = float(np.abs(e0[0] - e1[0]).max() / np.abs(e0[0]).max())
            row["log_evidence_diff"] = float(abs(e0[4] - e1[4]))
            row["every_output_equal"] = bool(all(np.array_equal(x, y) for x, y in zip(e0 + d0, e1 + d1)))
            out["shapes"][name]["S%d" % S] = row


def threshold():
    ctx = _lib.get_context()
    rng = np.random.default_rng(1)
    out["threshold"] = {}
    faster = {}
    for n in a.lengths:
        out["threshold"]["n%d" % n] = {}
        for S in a.states:
            C, off, logp, A, pi, qt, qp = problem(rng, 1, n, S)
            ch = _lib.Chain(ctx, C, off, S)
            try:
                ch.set(logp, A, pi, qt, qp, 1.0)
                ms, _ = alternated(ch, 1, {"expect": ch.expect}, 4 * a.steps, a.warmup)
            finally:
                ch.close()
            row = {route: stats(ms["expect"][route]) for route in ("off", "on")}
            row["off_over_on"] = row["off"]["median_ms"] / row["on"]["median_ms"]
            faster[n, S] = row["on"]["median_ms"] < row["off"]["median_ms"]
            out["threshold"]["n%d" % n]["S%d" % S] = row
    good = [n for n in sorted(a.lengths) if all(faster[m, S] for m in a.lengths if m >= n for S in a.states)]
    out["scan_from_measured"] = good[0] if good else None


for name, fn in (("shapes", shapes), ("threshold", threshold)):
    if name not in a.skip:
        fn()
print(json.dumps(out))
