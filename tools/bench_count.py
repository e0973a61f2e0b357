#!/usr/bin/env python3
"""Count-kernel microbenchmark (device-resident synthetic batch): ms per launch and algorithmic GB/s
(packed input + offsets + uint32 counts).  --lanes picks the count kernels (count_lanes; the table at PhkCountLanes,
csrc/phk_common.h): "" the library's choice, 0 the wave-per-contig kernel only, f the slot kernel whatever the batch looks
like, p / P the two-windows-per-add kernel with 512 / 1024 threads, q / Q the same whatever the batch looks like, d / D the
slot kernel with 512 / 1024 threads and no two-windows-per-add kernel; --invalid-ppm adds a validity mask; --ragged takes
heavy-tailed contig lengths (synth.ragged_lengths between --length and 100 x --length, as tools/diag/soak_ragged.py does).
`ms` sums the count kernels proper; `enqueue_ms` is the host time until the last of --iters back-to-back calls returns, with
the profile off and nothing waited for between them."""
import argparse, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from phamers_amd import _lib, device, synth

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=1000000)
ap.add_argument("--length", type=int, default=5000)
ap.add_argument("--k", type=int, default=4)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--invalid-ppm", type=int, default=0)
ap.add_argument("--check", type=int, default=64)
ap.add_argument("--ragged", action="store_true", help="heavy-tailed lengths in [--length, 100 x --length] instead of --length for all")
ap.add_argument("--lanes", default="", help="count_lanes knob: '' default, 0 wave-per-contig kernel only, f slot kernel forced, "
                "p / P two-windows-per-add kernel (512 / 1024 threads), q / Q the same forced, d / D slot kernel (512 / 1024 threads)")
a = ap.parse_args()
ctx = _lib.Context(0)
ctx.set_option("count_lanes", a.lanes)
n, L, k = a.contigs, a.length, a.k
D = 4 ** k
if a.ragged:
    lens = synth.ragged_lengths(1000, n, lo=L, hi=100 * L)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    T = int(offs[-1])
    off = device.DeviceArray.from_host(ctx, offs)
else:
    T = n * L
    off = device.DeviceArray(ctx, n + 1, np.uint64)
packed = device.DeviceArray(ctx, device.packed_words(T), np.uint32)
mask = device.DeviceArray(ctx, device.mask_words(T), np.uint32) if a.invalid_ppm else None
counts = device.DeviceArray(ctx, (n, D), np.uint32)
if a.ragged:
    device.synth_ragged(ctx, 1000, 0, n, off, T, packed, mask, gc_spread_permille=600, invalid_ppm=a.invalid_ppm)
else:
    device.synth_packed(ctx, 0, 0, n, L, packed, off, mask, a.invalid_ppm)
device.count(ctx, packed, mask, T, off, n, k, counts)
ctx.sync()
t0 = time.perf_counter()
for _ in range(a.iters):
    device.count(ctx, packed, mask, T, off, n, k, counts)
enqueue_ms = 1e3 * (time.perf_counter() - t0)
ctx.sync()
ctx.profile_reset(); ctx.profile_enable(True)
for _ in range(a.iters):
    device.count(ctx, packed, mask, T, off, n, k, counts)
ctx.sync()
prof = ctx.profile()
ms = sum(prof[name][0] for name in ("phk_count_kernel", "phk_count_pairs_kernel", "phk_count_direct_kernel") if name in prof) / a.iters
if a.ragged:
    alg = T // 4 + n * (8 + 4 * D) + (T // 8 if mask else 0)
else:
    alg = n * ((L + 3) // 4 + 8 + 4 * D) + (n * ((L + 7) // 8) if mask else 0)
ok = None
if a.check:
    from oracle import oracle
    m = min(a.check, n)
    if a.ragged:
        seqs = [synth.synth_ragged_contig(1000, c, int(lens[c]), 600, a.invalid_ppm) for c in range(m)]
    else:
        seqs = synth.synth_contigs(0, m, L, a.invalid_ppm)
    want = oracle.count(seqs, k).reshape(m, D)
    got = counts.rows_to_host(0, m).astype(np.int64)
    ok = bool(np.array_equal(got, want))
print(json.dumps({"lanes": a.lanes, "invalid_ppm": a.invalid_ppm, "ragged": a.ragged, "per_kernel_ms": {kn: v[0] / a.iters for kn, v in prof.items()},
                  "kernels": sorted(prof), "k": k, "contigs": n, "length": L, "total_bases": T, "iters": a.iters,
                  "ms": ms, "enqueue_ms": enqueue_ms, "GBps_algorithmic": alg / ms / 1e6, "Gbases_per_s": T / ms / 1e6,
                  "frac_hbm_peak": alg / ms / 1e6 / 8000.0, "bit_exact_vs_oracle": ok}))
