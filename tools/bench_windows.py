#!/usr/bin/env python3
"""
bench_windows.py -- sliding-window counts (phk_batch_windows_from_ascii, windows.hip) against the only route the package had
before: every window sliced out on the host and the slices counted as one batch (phk_batch_from_ascii), which moves and
counts every base window / step times.  k = 4, synthetic sequence (uniform ATGC), window 5000, steps 5000 / 500 / 50, once as
a few long sequences and once as many short ones.  Both routes are timed from host bytes (one uint8 buffer + offsets; the
slicing of the duplicate route is part of its time) to device-resident counts: a warm-up call, then --repeat timed calls,
best and spread (max - min) reported; the kernel times of one further call come from the library's event profile
(phk_profile_*).  One JSON line per (shape, step).  The duplicate route is skipped where its sliced bases would exceed
--dup-limit-gb.

Usage:  python tools/bench_windows.py [--mbases 128] [--repeat 5] [--steps 5000 500 50] [--dup-limit-gb 16]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K, WINDOW = 4, 5000


def timed(fn, repeat):
    fn()
    times = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t)
    return {"best_ms": 1e3 * min(times), "spread_ms": 1e3 * (max(times) - min(times)), "runs": repeat}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mbases', type=int, default=128)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--steps', type=int, nargs='+', default=[5000, 500, 50])
    ap.add_argument('--dup-limit-gb', type=float, default=16.0)
    args = ap.parse_args()
    from phamers_amd import _lib, kmer
    ctx = _lib.get_context()
    lib = ctx.lib
    total = args.mbases * 10 ** 6
    rng = np.random.RandomState(0)
    bases = np.frombuffer(b"ATGC", dtype=np.uint8)[rng.randint(0, 4, total).astype(np.uint8)]
    for shape, L in (("%d x 2 Mb" % (total // 2000000), 2000000), ("%d x 5 kb" % (total // 5000), 5000)):
        n = total // L
        lengths = np.full(n, L, dtype=np.int64)
        offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
        for step in args.steps:
            owner, start = kmer.window_plan(lengths, WINDOW, step)
            rows = owner.shape[0]
            line = {"shape": shape, "bases": int(offsets[-1]), "window": WINDOW, "step": step, "rows": rows}

            def new_route():
                h = ctypes.c_void_p()
                _lib.check(lib.phk_batch_windows_from_ascii(ctx.handle, _lib.ptr(bases), _lib.ptr(offsets), n, K, b"ATGC", WINDOW,
                                                            step, 0, ctypes.byref(h)))
                lib.phk_batch_free(ctx.handle, h)

            def dup_route():
                first = (offsets[owner].astype(np.int64) + start)
                sliced = np.lib.stride_tricks.sliding_window_view(bases, WINDOW)[first].reshape(-1)   # (a copy: rows x window bytes)
                dup_off = (np.arange(rows + 1, dtype=np.uint64) * np.uint64(WINDOW))
                h = ctypes.c_void_p()
                _lib.check(lib.phk_batch_from_ascii(ctx.handle, _lib.ptr(sliced), _lib.ptr(dup_off), rows, K, b"ATGC", ctypes.byref(h)))
                lib.phk_batch_free(ctx.handle, h)

            def kernels(fn):
                ctx.profile_enable(True)
                ctx.profile_reset()
                fn()
                prof = ctx.profile()
                ctx.profile_enable(False)
                return {name: round(ms, 4) for name, (ms, _) in sorted(prof.items()) if ms > 0}

            line["new"] = timed(new_route, args.repeat)
            line["new_kernels_ms"] = kernels(new_route)
            wk = line["new_kernels_ms"].get("phk_windows_lanes_kernel")
            if wk:
                line["row_write_GBps"] = rows * 4 ** K * 4 / wk / 1e6        # bytes of rows over the window kernel's time
            if rows * WINDOW <= args.dup_limit_gb * 2 ** 30:
                line["duplicate"] = timed(dup_route, max(2, args.repeat // 2) if rows * WINDOW > 2 ** 32 else args.repeat)
                line["duplicate_kernels_ms"] = kernels(dup_route)
            else:
                line["duplicate"] = "skipped: %.1f GB of sliced bases" % (rows * WINDOW / 2 ** 30)
            print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
