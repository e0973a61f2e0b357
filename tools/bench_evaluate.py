#!/usr/bin/env python3
"""
bench_evaluate.py -- learning.predictor_performance on the device against the host: the NumPy restatement of the integer
method (tests/evaluate_ref.py) and scikit-learn's roc_curve + auc, at n = 4 673 (the reference matrix), 2^20 and 10^8 scores.
The device call includes the upload; the resident form (phk_roc_curve_dev) is timed beside it.  One JSON line per size:
milliseconds (best of --repeat after a warm-up call), the sort's passes and the bytes they must move (32 B per key and pass
+ 20 B per key of preparation) over the resident time.

Usage:  python tools/bench_evaluate.py [--sizes 4673 1048576 100000000] [--repeat 5] [--no-host-above 20000000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def best(fn, repeat):
    fn()
    times = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t)
    return 1e3 * min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[4673, 1 << 20, 10 ** 8])
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--no-host-above', type=int, default=2 * 10 ** 7, help="skip the host comparisons above this n")
    args = ap.parse_args()
    from phamers_amd import _lib, device, learning
    from tests import evaluate_ref
    ctx = _lib.get_context()
    for n in args.sizes:
        rng = np.random.RandomState(1)
        scores = np.tanh(rng.normal(0.3, 1, n)) + rng.choice([-1.0, 1.0], n)       # combo-like
        labels = (rng.rand(n) < 0.5).astype(np.uint8)
        d_scores, d_labels = device.DeviceArray.from_host(ctx, scores), device.DeviceArray.from_host(ctx, labels)
        line = {"n": n, "repeat": args.repeat}
        line["device_with_upload_ms"] = best(lambda: learning.roc_points(scores, labels), args.repeat)
        line["device_resident_ms"] = best(lambda: learning.roc_points(None, None, _device=(d_scores.ptr, d_labels.ptr, n)), args.repeat)
        img = scores.view(np.uint64)
        passes = sum(1 for b in range(8) if len(np.unique((img >> np.uint64(8 * b)) & np.uint64(255))) > 1)   # (upper bound: sign folding aside)
        line["sort_passes_upper_bound"] = passes
        line["sort_bytes"] = n * (20 + 32 * passes)
        line["sort_bytes_over_resident_time_GBps"] = line["sort_bytes"] / line["device_resident_ms"] / 1e6
        if n <= args.no_host_above:
            from sklearn.metrics import auc, roc_curve

            def sk():
                f, t, _ = roc_curve(labels.astype(bool), scores)
                return auc(f, t)
            line["sklearn_host_ms"] = best(sk, max(1, args.repeat // 2))
            line["numpy_restatement_host_ms"] = best(lambda: evaluate_ref.roc_points(scores, labels), max(1, args.repeat // 2))
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
