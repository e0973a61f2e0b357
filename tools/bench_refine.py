#!/usr/bin/env python3
"""The boundary refinement against a NumPy restatement; one JSON line, and with ``--out DIR`` also
DIR/bench_refine.json and the tables of DIR/README.md (profiles/refine/).

boundaries  ``refine.boundaries`` (bases up, packed, one kernel, results down) against NumPy on the host -- the k-mer codes
            and their validity of the whole genome made once, outside the clock; per boundary a gather of the difference
            row, a cumulative sum and the arg-max under the tie rule -- alternated in one process, host clock, results
            asserted array_equal: ``--many`` boundaries of 1 000 bases at k = 4 and k = 6, and ``--long`` boundaries of 10^5
            bases at k = 4, on a random genome of ``--genome`` bases.  The kernel's own event time is reported beside.
segment     ``compose.segment_sequences`` on a synthetic genome of ``--genome`` bases in pieces of two base compositions,
            with and without ``refine=True``, alternated.
kernels     the resources of the refinement kernels from the code object (CPU only).
Nothing is promised; what was measured, and what was not, is written down.
"""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _codeobj, _lib, compose, refine, segment

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--genome", type=int, default=5000000)
ap.add_argument("--many", type=int, default=100000)
ap.add_argument("--long", type=int, default=2000)
ap.add_argument("--skip", nargs="*", default=[], choices=["boundaries", "segment", "kernels"])
ap.add_argument("--out", default=None, help="directory of bench_refine.json and README.md")
a = ap.parse_args()
out = {"workload": "refine", "genome": a.genome, "many": a.many, "long": a.long, "steps": a.steps}


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


def numpy_refine(code, valid, q, lo, x, hi, left, right):
    B = len(lo)
    pos, ev, sup = np.zeros(B, dtype=np.int64), np.zeros((B, 3), dtype=np.int64), np.zeros(B, dtype=np.int64)
    diff = {}
    for b in range(B):
        key = (int(left[b]), int(right[b]))
        if key not in diff:
            diff[key] = q[key[0]] - q[key[1]]
        v = valid[lo[b]:hi[b]]
        P = np.concatenate(([0], np.cumsum(np.where(v, diff[key][code[lo[b]:hi[b]]], 0))))
        at = np.flatnonzero(P == P.max()) + lo[b]
        p = at[np.lexsort((at, np.abs(at - x[b])))[0]]
        pos[b], sup[b] = p, int(v.sum())
        ev[b] = (P[p - lo[b]] - P[x[b] - lo[b]], P[p - lo[b]], P[p - lo[b]] - P[-1])
    return pos, ev, sup


def boundaries(ctx):
    rng = np.random.default_rng(0)
    digits = rng.integers(0, 4, a.genome).astype(np.int64)
    digits[rng.integers(0, a.genome, a.genome // 5000)] = 4                # scattered invalid bases
    seq = "".join(np.array(list("ATGCN"))[digits])
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
        ms = {"device": [], "numpy": []}
        for i in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            got = refine.boundaries([seq], k, logp, seqi, lo, x, hi, left, right)
            t1 = time.perf_counter()
            want = numpy_refine(code, valid, q, lo, x, hi, left, right)
            t2 = time.perf_counter()
            if i >= a.warmup:
                ms["device"].append((t1 - t0) * 1e3), ms["numpy"].append((t2 - t1) * 1e3)
        assert np.array_equal(got.position, want[0]) and np.array_equal(got.support, want[2])
        assert np.array_equal(np.stack([got.gain, got.left_evidence, got.right_evidence], axis=1), want[1])
        ctx.profile_reset()
        ctx.profile_enable(True)
        refine.boundaries([seq], k, logp, seqi, lo, x, hi, left, right)
        prof = {kk: v[0] for kk, v in ctx.profile().items()}
        ctx.profile_enable(False)
        row = {kk: stats(v) for kk, v in ms.items()}
        row.update(k=k, boundaries=int(B), bases_each=int(n), numpy_over_device=row["numpy"]["median_ms"] / row["device"]["median_ms"],
                   results_equal=True, kernel_ms=prof, moved=int((got.position != x).sum()))
        out["boundaries"][name] = row
        save()


def segment_bench():
    rng = np.random.default_rng(1)
    piece = 50000
    freqs = [np.array([0.32, 0.32, 0.18, 0.18]), np.array([0.22, 0.22, 0.28, 0.28])]
    cuts = np.arange(0, a.genome, piece) + np.concatenate(([0], rng.integers(-200, 200, (a.genome - 1) // piece)))
    parts = [rng.choice(4, int(e - s), p=freqs[i % 2]) for i, (s, e) in enumerate(zip(cuts, np.concatenate((cuts[1:], [a.genome]))))]
    seq = "".join(np.array(list("ATGC"))[np.concatenate(parts)])
    ms = {"plain": [], "refined": []}
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        plain = compose.segment_sequences([seq], 2, max_iter=20)
        t1 = time.perf_counter()
        fine = compose.segment_sequences([seq], 2, max_iter=20, refine=True)
        t2 = time.perf_counter()
        if i >= a.warmup:
            ms["plain"].append((t1 - t0) * 1e3), ms["refined"].append((t2 - t1) * 1e3)
    assert np.array_equal(plain.state, fine.state)
    b = fine.boundaries
    row = {kk: stats(v) for kk, v in ms.items()}
    row.update(windows=len(fine), boundaries=len(b.position), true_changes=len(cuts) - 1)
    if len(b.position):
        true = cuts[1:]
        near = lambda v: np.abs(np.asarray(v)[:, None] - true[None, :]).min(axis=1)
        row.update(median_distance_refined=float(np.median(near(b.position))), median_distance_grid=float(np.median(near(b.window_boundary))))
    out["segment"] = row
    save()


def kernels():
    res = _codeobj.kernel_resources(_lib.LIB_PATH)
    out["kernels"] = {name: {kk: int(r[kk]) for kk in ("vgpr_count", "scratch_bytes", "lds_bytes", "vgpr_spill_count")}
                      for name, r in sorted(res.items()) if "phk_refine_" in name}


def save():
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench_refine.json"), "w") as f:
            json.dump(out, f)


def readme():
    L = ["## Measured", "", "Written by `tools/bench_refine.py --out profiles/refine` (the numbers: bench_refine.json).", ""]
    if "boundaries" in out:
        L += ["### `refine.boundaries` against NumPy on the host (genome of %d bases, results array_equal)" % a.genome, "",
              "| shape | k | boundaries x bases | device call, ms (median; min..max) | kernel event, ms | NumPy, ms | NumPy / device |",
              "|---|---|---|---|---|---|---|"]
        for name, r in out["boundaries"].items():
            L.append("| %s | %d | %d x %d | %.2f (%.2f..%.2f) | %.3f | %.0f | %.0f |" % (
                name, r["k"], r["boundaries"], r["bases_each"], r["device"]["median_ms"], r["device"]["min_ms"], r["device"]["max_ms"],
                r["kernel_ms"].get("phk_refine_boundaries_kernel", float("nan")), r["numpy"]["median_ms"], r["numpy_over_device"]))
        L.append("")
    if "segment" in out:
        r = out["segment"]
        L += ["### `segment_sequences` on a synthetic genome of %d bases (%d windows), S = 2" % (a.genome, r["windows"]), "",
              "| without refine, ms | with refine=True, ms | boundaries | true change points | median distance to a true change: refined / grid |",
              "|---|---|---|---|---|",
              "| %.0f | %.0f | %d | %d | %s / %s |" % (r["plain"]["median_ms"], r["refined"]["median_ms"], r["boundaries"], r["true_changes"],
                                                     r.get("median_distance_refined", "-"), r.get("median_distance_grid", "-")), ""]
    if "kernels" in out:
        L += ["### The kernels in this build (code object)", "", "| kernel | VGPRs | scratch | LDS |", "|---|---|---|---|"]
        L += ["| `%s` | %d | %d | %d |" % (kk, r["vgpr_count"], r["scratch_bytes"], r["lds_bytes"]) for kk, r in out["kernels"].items()]
        L.append("")
    return "\n".join(L)


if "kernels" not in a.skip:
    kernels()
if "boundaries" not in a.skip:
    boundaries(_lib.get_context())
if "segment" not in a.skip:
    segment_bench()
save()
if a.out:
    path = os.path.join(a.out, "README.md")
    head = open(path).read().split("## Measured")[0] if os.path.exists(path) else ""
    with open(path, "w") as f:
        f.write(head + readme())
print(json.dumps(out))
