#!/usr/bin/env python3
"""The boundary confidence against ``refine.boundaries`` alone and against a NumPy restatement; one
JSON line, and with ``--out DIR`` also DIR/bench_refine_confidence.json and the tables of DIR/README.md
(profiles/refine_confidence/).

On the two shapes of tools/bench_refine.py -- ``--many`` boundaries of 1 000 bases at k = 4 and k = 6, ``--long`` boundaries
of 10^5 bases at k = 4, on a random genome of ``--genome`` bases -- three things alternated in one process under the host
clock: ``refine.confidence`` (bases up, packed, two kernels, results down, the host's ratios), ``refine.boundaries`` (the
same with one kernel) and NumPy on the host (the k-mer codes of the genome made once, outside the clock; per boundary a
gather, a cumulative sum, the arg-max, the threshold and the five float64 sums).  The integers are asserted array_equal, the
sums equal within (n + 8) 2^-52 relative.  The kernels' own event times are reported beside.  Nothing is promised.
"""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _codeobj, _lib, refine, segment

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--genome", type=int, default=5000000)
ap.add_argument("--many", type=int, default=100000)
ap.add_argument("--long", type=int, default=2000)
ap.add_argument("--drop", type=float, default=3.0)
ap.add_argument("--out", default=None, help="directory of bench_refine_confidence.json and README.md")
a = ap.parse_args()
out = {"workload": "refine_confidence", "genome": a.genome, "many": a.many, "long": a.long, "steps": a.steps, "drop": a.drop}
CUT = 700 << 16


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def codes_of(digits, k):
    """(codes (L,) int64, valid (L,) bool) of every k-mer start of a sequence given as digits 0..3 (4: no symbol)."""
    L = len(digits)
    ok = digits < 4
    code, valid = np.zeros(L, dtype=np.int64), np.ones(L, dtype=bool)
    for j in range(k):
        code[:L - j] = code[:L - j] * 4 + np.where(ok[j:], digits[j:], 0)
        valid[:L - j] &= ok[j:]
        if j:
            valid[L - j:] = False
    return code, valid


def numpy_confidence(code, valid, q, lo, x, hi, left, right, drop_q):
    B = len(lo)
    pos, interval, sums = np.zeros(B, dtype=np.int64), np.zeros((B, 3), dtype=np.int64), np.zeros((B, 5))
    diff = {}
    for b in range(B):
        key = (int(left[b]), int(right[b]))
        if key not in diff:
            diff[key] = q[key[0]] - q[key[1]]
        P = np.concatenate(([0], np.cumsum(np.where(valid[lo[b]:hi[b]], diff[key][code[lo[b]:hi[b]]], 0))))
        at = np.flatnonzero(P == P.max()) + lo[b]
        p = at[np.lexsort((at, np.abs(at - x[b])))[0]]
        delta = P[p - lo[b]] - P
        inside = np.flatnonzero(delta <= drop_q)
        w = np.where(delta <= CUT, np.exp(-(np.minimum(delta, CUT) * 2.0 ** -16)), 0.0)
        off = np.arange(lo[b], hi[b] + 1) - p
        pos[b], interval[b] = p, (lo[b] + inside[0], lo[b] + inside[-1], len(inside))
        sums[b] = (w.sum(), w[inside[0]:inside[-1] + 1].sum(), (-off[off < 0] * w[off < 0]).sum(), (off[off > 0] * w[off > 0]).sum(),
                   ((off * off) * w).sum())
    return pos, interval, sums


def kernels():
    res = _codeobj.kernel_resources(_lib.LIB_PATH)
    out["kernels"] = {name: {kk: int(r[kk]) for kk in ("vgpr_count", "scratch_bytes", "lds_bytes", "vgpr_spill_count")}
                      for name, r in sorted(res.items()) if "phk_refine_" in name or "phk_boundary_confidence" in name}


def boundaries(ctx):
    rng = np.random.default_rng(0)
    digits = rng.integers(0, 4, a.genome).astype(np.int64)
    digits[rng.integers(0, a.genome, a.genome // 5000)] = 4                # scattered invalid bases
    seq = "".join(np.array(list("ATGCN"))[digits])
    drop_q = refine.drop_quantum(a.drop)
    out["boundaries"] = {}
    for name, k, B, n in (("many_k4", 4, a.many, 1000), ("many_k6", 6, a.many, 1000), ("long_k4", 4, a.long, 100000)):
        n = min(n, a.genome // 2)
        logp = np.log(rng.dirichlet(np.full(4 ** k, 5.0), 4))
        q = segment.quantise(logp)
        lo = rng.integers(0, a.genome - n, B)
        hi = lo + n
        x = lo + rng.integers(0, n + 1, B)
        left = rng.integers(0, 4, B)
        right = (left + 1 + rng.integers(0, 3, B)) % 4
        code, valid = codes_of(digits, k)
        seqi = np.zeros(B, dtype=np.int64)
        ms = {"confidence": [], "boundaries": [], "numpy": []}
        for i in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            r, c = refine.confidence([seq], k, logp, seqi, lo, x, hi, left, right, drop=a.drop)
            t1 = time.perf_counter()
            plain = refine.boundaries([seq], k, logp, seqi, lo, x, hi, left, right)
            t2 = time.perf_counter()
            if i >= a.warmup:
                ms["confidence"].append((t1 - t0) * 1e3), ms["boundaries"].append((t2 - t1) * 1e3)
        t2 = time.perf_counter()                                           # (seconds a call: once is enough)
        want = numpy_confidence(code, valid, q, lo, x, hi, left, right, drop_q)
        ms["numpy"].append((time.perf_counter() - t2) * 1e3)
        assert all(np.array_equal(g, w) for g, w in zip(r, plain))
        assert np.array_equal(r.position, want[0]) and np.array_equal(np.stack([c.lower, c.upper, c.n_within], axis=1), want[1])
        rel = np.abs(c.sums - want[2]) / np.where(want[2] > 0, want[2], 1.0)
        assert (rel <= (n + 9) * 2.0 ** -52).all(), float(rel.max())
        ctx.profile_reset()
        ctx.profile_enable(True)
        refine.confidence([seq], k, logp, seqi, lo, x, hi, left, right, drop=a.drop)
        prof = {kk: v[0] for kk, v in ctx.profile().items()}
        ctx.profile_enable(False)
        row = {kk: stats(v) for kk, v in ms.items()}
        row.update(k=k, boundaries=int(B), bases_each=int(n), numpy_over_confidence=row["numpy"]["median_ms"] / row["confidence"]["median_ms"],
                   confidence_over_boundaries=row["confidence"]["median_ms"] / row["boundaries"]["median_ms"], results_equal=True,
                   kernel_ms=prof, median_width=float(np.median(c.upper - c.lower)), median_mass_within=float(np.median(c.mass_within)),
                   cut_short=int((c.at_lo | c.at_hi).sum()), worst_relative_difference_of_a_sum=float(rel.max()))
        out["boundaries"][name] = row
        save()


def save():
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench_refine_confidence.json"), "w") as f:
            json.dump(out, f)


def readme():
    L = ["## Measured", "", "Written by `tools/bench_refine_confidence.py --out profiles/refine_confidence` (the numbers: "
         "bench_refine_confidence.json).", ""]
    if "boundaries" in out:
        L += ["### `refine.confidence` against `refine.boundaries` and NumPy (genome of %d bases, drop = %g nats, results equal)"
              % (a.genome, a.drop), "",
              "| shape | k | boundaries x bases | confidence call, ms (median; min..max) | boundaries call, ms | ratio | "
              "refinement kernel, ms | confidence kernel, ms | NumPy, ms | NumPy / confidence |", "|---|---|---|---|---|---|---|---|---|---|"]
        for name, r in out["boundaries"].items():
            L.append("| %s | %d | %d x %d | %.2f (%.2f..%.2f) | %.2f | %.2f | %.3f | %.3f | %.0f | %.0f |" % (
                name, r["k"], r["boundaries"], r["bases_each"], r["confidence"]["median_ms"], r["confidence"]["min_ms"],
                r["confidence"]["max_ms"], r["boundaries"]["median_ms"], r["confidence_over_boundaries"],
                r["kernel_ms"].get("phk_refine_boundaries_kernel", float("nan")),
                r["kernel_ms"].get("phk_boundary_confidence_kernel", float("nan")), r["numpy"]["median_ms"], r["numpy_over_confidence"]))
        L.append("")
    if "kernels" in out:
        L += ["### The kernels in this build (code object)", "", "| kernel | VGPRs | scratch | LDS |", "|---|---|---|---|"]
        L += ["| `%s` | %d | %d | %d |" % (kk, r["vgpr_count"], r["scratch_bytes"], r["lds_bytes"]) for kk, r in out["kernels"].items()]
        L.append("")
    return "\n".join(L)


kernels()
boundaries(_lib.get_context())
save()
if a.out:
    path = os.path.join(a.out, "README.md")
    head = open(path).read().split("## Measured")[0] if os.path.exists(path) else ""
    with open(path, "w") as f:
        f.write(head + readme())
print(json.dumps(out))
