#!/usr/bin/env python3
"""Grouped chains against the per-scaffold loop of the API they extend; one JSON line, and with
``--out DIR`` also DIR/bench_compose_groups.json and the tables of DIR/README.md (profiles/compose_groups/).

assembly   a synthetic assembly of ``--scaffolds`` scaffolds of 40 to 400 windows (window = step = 500: 497 4-mers a window,
           D = 256; every scaffold two to four pieces drawn from three compositions of its own), rows resident, at
           S = 2, 3, 8:
  estep    one grouped E-step (``Chain.set_grouped`` + ``expect_grouped``, one group per scaffold) against the sum of the
           per-scaffold ``Chain.set`` + ``expect`` calls on chains made once from each scaffold's rows; alternated in one
           process, host clock around calls that end with their results on the host; results asserted array_equal.
  fit      a whole ``compose.fit_groups`` against the loop of ``compose.fit`` per scaffold (``--max_iter`` M-steps at the
           most, the same on both sides), alternated; Compositions asserted array_equal; the share of the grouped call
           spent in the host M-step (``compose.m_step`` timed inside the call).
many       ``--groups`` groups of one 20-window record against the shared-parameter E-step (``Chain.set`` + ``expect``) of
           the same rows: what per-group parameters, per-group results and idle emission tiles cost.
kernels    the VGPR counts of the chain kernels from the code object (CPU only).
The loop and the shared-parameter call are the yardsticks; nothing is promised, what loses is written down.
"""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _codeobj, _lib, compose, segment

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--scaffolds", type=int, default=2000)
ap.add_argument("--groups", type=int, default=100000, help="groups of the many-groups shape")
ap.add_argument("--states", type=int, nargs="*", default=[2, 3, 8])
ap.add_argument("--max_iter", type=int, default=20, help="most M-steps of the timed fits")
ap.add_argument("--fit_reps", type=int, default=1)
ap.add_argument("--skip", nargs="*", default=[], choices=["estep", "fit", "many", "kernels"])
ap.add_argument("--out", default=None, help="directory of bench_compose_groups.json and README.md")
ap.add_argument("--readme_from", default=None, help="write --out/README.md from this JSON of an earlier run; measures nothing")
a = ap.parse_args()
D, KMERS = 256, 497
out = {"workload": "compose_groups", "D": D, "scaffolds": a.scaffolds, "groups": a.groups, "states": a.states,
       "max_iter": a.max_iter}


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "calls_ms": [float(m) for m in ms]}


def assembly(rng, R):
    """(counts (n, D) uint32, offsets (R + 1,)): scaffold r has 40 .. 400 windows in 2 .. 4 pieces from 3 compositions."""
    lengths = rng.integers(40, 401, R)
    base = rng.dirichlet(np.full(D, 8.0))
    parts = []
    for n in lengths:
        own = [(lambda p: p / p.sum())(base * np.exp(0.45 * rng.standard_normal(D))) for _ in range(3)]
        cuts = np.sort(rng.choice(np.arange(10, n - 9), rng.integers(1, 4), replace=False))
        for i, (lo, hi) in enumerate(zip(np.concatenate(([0], cuts)), np.concatenate((cuts, [n])))):
            parts.append(rng.multinomial(KMERS, own[i % 3], int(hi - lo)))
    return np.vstack(parts).astype(np.uint32), np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)


def parameters(rng, G, S):
    logp = np.log(rng.dirichlet(np.full(D, 20.0), (G, S)))
    A, pi = compose.start_chain(S)
    A, pi = np.tile(A, (G, 1, 1)), np.tile(pi, (G, 1))
    return logp, A, pi, segment.quantise(np.log(A)), segment.quantise(np.log(pi))


def save():
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench_compose_groups.json"), "w") as f:
            json.dump(out, f)


def estep(ctx, C, off):
    R = len(off) - 1
    rng = np.random.default_rng(1)
    out["estep"] = {"windows": int(off[-1])}
    batch = _lib.Batch.from_counts(ctx, C)
    for S in a.states:
        logp, A, pi, qt, qp = parameters(rng, R, S)
        grouped = _lib.Chain(ctx, batch, off, S)
        grouped.set_groups(np.arange(R + 1, dtype=np.uint64))
        alone = [_lib.Chain(ctx, C[int(off[r]):int(off[r + 1])], [0, int(off[r + 1] - off[r])], S) for r in range(R)]
        ms = {"grouped": [], "loop": []}
        try:
            for i in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                grouped.set_grouped(logp, A, pi, qt, qp, 1.0)
                got = grouped.expect_grouped()
                t1 = time.perf_counter()
                want = []
                for r, ch in enumerate(alone):
                    ch.set(logp[r], A[r], pi[r], qt[r], qp[r], 1.0)
                    want.append(ch.expect())
                t2 = time.perf_counter()
                if i >= a.warmup:
                    ms["grouped"].append((t1 - t0) * 1e3), ms["loop"].append((t2 - t1) * 1e3)
            for k in range(5):
                assert np.array_equal(got[k], np.array([w[k] for w in want])), (S, k)
            ctx.profile_reset()
            ctx.profile_enable(True)
            grouped.set_grouped(logp, A, pi, qt, qp, 1.0)
            grouped.expect_grouped()
            prof = {k: v[0] for k, v in ctx.profile().items()}
            ctx.profile_enable(False)
        finally:
            grouped.close()
            for ch in alone:
                ch.close()
        row = {k: stats(v) for k, v in ms.items()}
        row["loop_over_grouped"] = row["loop"]["median_ms"] / row["grouped"]["median_ms"]
        row["results_equal"] = True
        row["grouped_kernel_ms"] = prof
        out["estep"]["S%d" % S] = row
        save()
    batch.close()


def fit(ctx, C, off):
    R = len(off) - 1
    out["fit"] = {}
    groups = np.arange(R + 1, dtype=np.uint64)
    batch = _lib.Batch.from_counts(ctx, C)
    spent = [0.0]
    inner = compose.m_step

    def timed_m_step(*args, **kw):
        t0 = time.perf_counter()
        r = inner(*args, **kw)
        spent[0] += time.perf_counter() - t0
        return r

    compose.fit_groups(C[:int(off[8])], off[:9], groups[:9], 2, max_iter=2)          # warm-up: first launches, allocations
    for S in a.states:
        ms = {"grouped": [], "loop": [], "m_step_in_grouped": []}
        for i in range(a.fit_reps):
            compose.m_step, spent[0] = timed_m_step, 0.0
            t0 = time.perf_counter()
            got = compose.fit_groups(batch, off, groups, S, max_iter=a.max_iter)
            t1 = time.perf_counter()
            compose.m_step = inner
            want = []
            for r in range(R):
                rows = C[int(off[r]):int(off[r + 1])]
                want.append(compose.fit(rows, [0, len(rows)], S, max_iter=a.max_iter) if got.status[r] == compose.GROUP_FITTED else None)
            t2 = time.perf_counter()
            ms["grouped"].append((t1 - t0) * 1e3), ms["loop"].append((t2 - t1) * 1e3), ms["m_step_in_grouped"].append(spent[0] * 1e3)
        for r in range(R):
            assert (got[r] is None) == (want[r] is None)
            if got[r] is not None:
                for name in ("log_profiles", "trans", "init", "occupancy", "expected_counts", "trace"):
                    assert np.array_equal(getattr(got[r], name), getattr(want[r], name)), (S, r, name)
        row = {k: stats(v) for k, v in ms.items()}
        row["loop_over_grouped"] = row["loop"]["median_ms"] / row["grouped"]["median_ms"]
        row["m_step_share_of_grouped"] = row["m_step_in_grouped"]["median_ms"] / row["grouped"]["median_ms"]
        row["fitted"], row["too_short"] = int((got.status == 0).sum()), int((got.status == 1).sum())
        row["iterations_total"], row["iterations_most"] = int(got.n_iter.sum()), int(got.n_iter.max())
        row["device_calls_grouped"] = int(got.n_iter.max()) + 1
        row["results_equal"] = True
        out["fit"]["S%d" % S] = row
        save()
    batch.close()


def many(ctx):
    G, n = a.groups, 20
    rng = np.random.default_rng(2)
    out["many"] = {"groups": G, "windows_per_group": n}
    C = rng.integers(0, 4, (G * n, D), dtype=np.uint8).astype(np.uint32)
    off = np.arange(G + 1, dtype=np.uint64) * np.uint64(n)
    for S in a.states:
        logp, A, pi, qt, qp = parameters(rng, 1, S)
        ch = _lib.Chain(ctx, C, off, S)
        ms = {"shared": [], "grouped": []}
        try:
            glogp, gA, gpi = np.tile(logp, (G, 1, 1)), np.tile(A, (G, 1, 1)), np.tile(pi, (G, 1))
            gqt, gqp = np.tile(qt, (G, 1, 1)), np.tile(qp, (G, 1))
            for i in range(a.warmup + a.steps):
                ch.set_groups(None)
                t0 = time.perf_counter()
                ch.set(logp[0], A[0], pi[0], qt[0], qp[0], 1.0)
                shared = ch.expect(records=True)
                t1 = time.perf_counter()
                ch.set_groups(np.arange(G + 1, dtype=np.uint64))
                t2 = time.perf_counter()
                ch.set_grouped(glogp, gA, gpi, gqt, gqp, 1.0)
                got = ch.expect_grouped()
                t3 = time.perf_counter()
                if i >= a.warmup:
                    ms["shared"].append((t1 - t0) * 1e3), ms["grouped"].append((t3 - t2) * 1e3)
            assert np.array_equal(got[4], shared[5])                  # a group of one record: its evidence is the record's
            ctx.profile_reset()
            ctx.profile_enable(True)
            ch.set_grouped(glogp, gA, gpi, gqt, gqp, 1.0)
            ch.expect_grouped()
            prof = {k: v[0] for k, v in ctx.profile().items()}
            ctx.profile_enable(False)
        finally:
            ch.close()
        row = {k: stats(v) for k, v in ms.items()}
        row["grouped_over_shared"] = row["grouped"]["median_ms"] / row["shared"]["median_ms"]
        row["grouped_kernel_ms"] = prof
        row["result_bytes_grouped"] = int(sum(x.nbytes for x in got))
        out["many"]["S%d" % S] = row
        save()


def kernels():
    res = _codeobj.kernel_resources(_lib.LIB_PATH)
    out["kernels"] = {name: {k: int(r[k]) for k in ("vgpr_count", "scratch_bytes", "lds_bytes", "vgpr_spill_count")}
                      for name, r in sorted(res.items()) if "phk_chain_" in name and "_scan_" not in name}


def readme():
    L = ["## Measured", "",
         "Written by `tools/bench_compose_groups.py --out profiles/compose_groups` (the numbers: bench_compose_groups.json).", ""]
    if "estep" in out:
        L += ["### One E-step: %d scaffolds, %d windows, one group per scaffold" % (a.scaffolds, out["estep"]["windows"]), "",
              "| S | grouped call, ms (median; min..max) | per-scaffold loop, ms | loop / grouped |", "|---|---|---|---|"]
        for S in a.states:
            r = out["estep"]["S%d" % S]
            L.append("| %d | %.2f (%.2f..%.2f) | %.1f (%.1f..%.1f) | %.1f |" % (
                S, r["grouped"]["median_ms"], r["grouped"]["min_ms"], r["grouped"]["max_ms"], r["loop"]["median_ms"],
                r["loop"]["min_ms"], r["loop"]["max_ms"], r["loop_over_grouped"]))
        L += ["", "Kernel event times of one grouped call, ms:", ""]
        for S in a.states:
            L.append("- S = %d: %s" % (S, ", ".join("%s %.3f" % (k.replace("phk_chain_", ""), v) for k, v in
                                                   sorted(out["estep"]["S%d" % S]["grouped_kernel_ms"].items()))))
        L.append("")
    if "fit" in out:
        L += ["### A whole fit (at most %d M-steps), fit_groups against the loop of fit" % a.max_iter, "",
              "| S | fit_groups, ms | loop of fit, ms | loop / grouped | host M-step share of fit_groups | fitted / too short | device calls grouped | E-steps of the loop |",
              "|---|---|---|---|---|---|---|---|"]
        for S in a.states:
            r = out["fit"]["S%d" % S]
            L.append("| %d | %.0f | %.0f | %.1f | %.0f %% | %d / %d | %d | %d |" % (
                S, r["grouped"]["median_ms"], r["loop"]["median_ms"], r["loop_over_grouped"], 100 * r["m_step_share_of_grouped"],
                r["fitted"], r["too_short"], r["device_calls_grouped"], r["iterations_total"] + r["fitted"]))
        L.append("")
    if "many" in out:
        L += ["### %d groups of one 20-window record against the shared-parameter E-step of the same rows" % a.groups, "",
              "| S | shared parameters, ms | grouped, ms | grouped / shared | bytes of results to the host, grouped |", "|---|---|---|---|---|"]
        for S in a.states:
            r = out["many"]["S%d" % S]
            L.append("| %d | %.1f | %.1f | %.1f | %d |" % (S, r["shared"]["median_ms"], r["grouped"]["median_ms"],
                                                         r["grouped_over_shared"], r["result_bytes_grouped"]))
        L += ["", "Kernel event times of one grouped call, ms:", ""]
        for S in a.states:
            L.append("- S = %d: %s" % (S, ", ".join("%s %.3f" % (k.replace("phk_chain_", ""), v) for k, v in
                                                   sorted(out["many"]["S%d" % S]["grouped_kernel_ms"].items()))))
        L.append("")
    if "kernels" in out:
        L += ["### VGPRs of the chain kernels in this build (code object)", "", "| kernel | VGPRs | scratch | LDS |", "|---|---|---|---|"]
        L += ["| `%s` | %d | %d | %d |" % (k, r["vgpr_count"], r["scratch_bytes"], r["lds_bytes"]) for k, r in out["kernels"].items()]
        L.append("")
    return "\n".join(L)


if a.readme_from:
    out = json.load(open(a.readme_from))
    a.scaffolds, a.groups, a.states, a.max_iter = out["scaffolds"], out["groups"], out["states"], out["max_iter"]
    a.skip = ["estep", "fit", "many", "kernels"]
ctx = None
if set(("estep", "fit", "many")) - set(a.skip):
    ctx = _lib.get_context()
    C, off = assembly(np.random.default_rng(0), a.scaffolds)
if "kernels" not in a.skip:
    kernels()
for name, fn in (("estep", lambda: estep(ctx, C, off)), ("fit", lambda: fit(ctx, C, off)), ("many", lambda: many(ctx))):
    if name not in a.skip:
        fn()
if not a.readme_from:
    save()
if a.out:
    path = os.path.join(a.out, "README.md")
    head = open(path).read().split("## Measured")[0] if os.path.exists(path) else ""
    with open(path, "w") as f:
        f.write(head + readme())
print(json.dumps(out))
