#!/usr/bin/env python
"""ON THE GPU BOX: what the host driver of phk_count_score_dev costs, one library per process (A/B against another build:
PHAMERS_AB_LIB with PHK_ALLOW_DIAGNOSTIC_BUILD=1, as tools/diag/ab_bench.sh does).  At a bench.py configuration's shape:

  sync_ms_per_step   median over --sync-steps steps of one count_score call + a wait for the device
  enqueue_ms         host time until the LAST of --steps back-to-back count_score calls returns, nothing waited for between
                     them (then the device is drained: drain_ms)

--trace-steps N instead: warm up, wait, N steps, wait, leave -- the block between the last two waits is what a HIP API trace
of the process (rocprofv3 --hip-runtime-trace) shows as N steady-state steps.  One JSON line on stdout.

    python tools/diag/score_driver_ab.py --config 1 [--contigs N] [--score-batch B] [--steps 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from phamers_amd import _lib, device, workloads   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=1, choices=[1, 2, 4])
    ap.add_argument("--contigs", type=int, default=None)
    ap.add_argument("--score-batch", type=int, default=0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--sync-steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-steps", type=int, default=0)
    args = ap.parse_args()
    cfg = workloads.CONFIGS[args.config]
    k, L, n = cfg["k"], cfg["length"], args.contigs or cfg["contigs"]
    T = n * L
    ctx = _lib.Context(_lib.default_device())
    pos, neg, cpos, cneg, _ = workloads.reference_for(ctx, cfg, None)
    model = _lib.Model(ctx, pos, neg, cpos, cneg, k_neighbors=3)
    d_packed = device.DeviceArray(ctx, device.packed_words(T), np.uint32)
    d_off = device.DeviceArray(ctx, n + 1, np.uint64)
    d_counts = device.DeviceArray(ctx, (n, 4 ** k), np.uint32)
    d_scores = device.DeviceArray(ctx, n, np.float64)
    d_status = device.DeviceArray(ctx, 1, np.uint32)
    device.synth_packed(ctx, 0, 0, n, L, d_packed, d_off)
    if args.score_batch:
        ctx.set_option("score_batch", str(args.score_batch))

    def step():
        device.count_score(ctx, model, d_packed, None, T, d_off, n, k, "combo", d_counts, d_scores, d_status)

    for _ in range(args.warmup):
        step()
    ctx.sync()
    out = {"lib": os.environ.get("PHAMERS_AB_LIB") or "in-tree", "config": args.config, "contigs": n, "score_batch": args.score_batch}
    if args.trace_steps:
        for _ in range(args.trace_steps):
            step()
        ctx.sync()
        out["traced_steps"] = args.trace_steps
    else:
        times = []
        for _ in range(args.sync_steps):
            t0 = time.perf_counter()
            step()
            ctx.sync()
            times.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        t1 = time.perf_counter()
        ctx.sync()
        t2 = time.perf_counter()
        out.update(sync_ms_per_step=1e3 * float(np.median(times)), steps=args.steps, enqueue_ms=1e3 * (t1 - t0),
                   drain_ms=1e3 * (t2 - t1))
    print(json.dumps(out))
    sys.stdout.flush()
    model.close()
    ctx.close()


if __name__ == "__main__":
    main()
