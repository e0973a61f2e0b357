#!/usr/bin/env python3
"""
bench_strands.py -- the strand fold (phk_batch_fold_strands, strands.hip) on resident batches: its kernel time beside the
time of the count kernels that produced the same batch, both from the library's event profile (phk_profile_*), and the
fold's traffic -- every count word read once and written once, 2 n 4^k 4 bytes -- over its kernel time, against the
6.3 TB/s a streaming copy reaches on an MI355X (of 8 TB/s peak).  Synthetic uniform ATGC; the shapes are 2^20 rows at
k = 4, 2^18 at k = 5 and 2^16 at k = 6 (1 GiB of counts each).  A batch can be folded once, so every repeat builds the
batch anew; best and spread (max - min) over --repeat builds, one JSON line per shape.

With --cross-validate POSITIVE.csv NEGATIVE.csv: the N-fold cross-validation AUC of --method on the two feature files,
forward counts and folded counts, same seeded fold plan (one more JSON line); the same .npz given twice is read as
tests/golden/ref_features.npz (pos_counts / neg_counts).

Usage:  python tools/bench_strands.py [--repeat 3] [--shapes 4:20 5:18 6:16] [--bases-per-row-k4 500]
                                      [--cross-validate PF NF [--folds 20 --method combo --seed 0]]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_ACHIEVABLE_GBPS = 6300.0


def fold_shape(ctx, bases, k, log2_rows, repeat):
    from phamers_amd import _lib
    n = 1 << log2_rows
    L = bases.shape[0] // n
    offsets = (np.arange(n + 1, dtype=np.uint64) * np.uint64(L))
    fold_ms, count_ms, check_ms = [], [], []
    for _ in range(repeat + 1):            # (the first build warms up: code objects, workspaces)
        ctx.profile_enable(True)
        ctx.profile_reset()
        h = ctypes.c_void_p()
        _lib.check(ctx.lib.phk_batch_from_ascii(ctx.handle, _lib.ptr(bases), _lib.ptr(offsets), n, k, b"ATGC", ctypes.byref(h)))
        b = _lib.Batch(ctx, h)
        try:
            b.fold_strands()
            prof = ctx.profile()
            sums = b.row_sums()
        finally:
            b.close()
            ctx.profile_enable(False)
        assert (sums == 2 * (L - k + 1)).all()
        fold_ms.append(prof["phk_fold_strands_kernel"][0])
        check_ms.append(prof["phk_fold_check_kernel"][0])
        count_ms.append(sum(ms for name, (ms, _) in prof.items() if name.startswith("phk_count_")))
    fold_ms, count_ms, check_ms = fold_ms[1:], count_ms[1:], check_ms[1:]
    traffic = 2 * n * 4 ** k * 4
    best = min(fold_ms)
    return {"k": k, "rows": n, "bases_per_row": L, "count_bytes": n * 4 ** k * 4,
            "fold_kernel_ms": {"best": round(best, 4), "spread": round(max(fold_ms) - best, 4), "runs": repeat},
            "fold_check_kernel_ms": round(min(check_ms), 4),
            "count_kernels_ms": {"best": round(min(count_ms), 4), "spread": round(max(count_ms) - min(count_ms), 4)},
            "fold_GBps": round(traffic / best / 1e6, 1),
            "fold_fraction_of_achievable_hbm": round(traffic / best / 1e6 / HBM_ACHIEVABLE_GBPS, 3),
            "kernels_ms_last_run": {name: round(ms, 4) for name, (ms, _) in sorted(prof.items()) if ms > 0}}


def cross_validation_auc(pf, nf, folds, method, seed):
    from phamers_amd import cross_validate, fileIO, kmer, learning, transform_kmers
    if pf == nf and pf.endswith(".npz"):       # tests/golden/ref_features.npz: both matrices in one file
        with np.load(pf) as z:
            pos, neg = z["pos_counts"].astype(np.int64), z["neg_counts"].astype(np.int64)
    else:
        _, pos = fileIO.read_feature_file(pf)
        _, neg = fileIO.read_feature_file(nf)
    out = {"cross_validation": {"positive": os.path.basename(pf), "negative": os.path.basename(nf), "folds": folds,
                                "method": method, "seed": seed, "rows": [int(pos.shape[0]), int(neg.shape[0])]}}
    for name, fn in (("forward", lambda c: c), ("both_strands", transform_kmers.fold_strands)):
        v = cross_validate.cross_validator()
        v.method, v.N, v.seed = method, folds, seed
        v.positive_data, v.negative_data = kmer.normalize_counts(fn(pos)), kmer.normalize_counts(fn(neg))
        p, q = v.cross_validate()
        out["cross_validation"]["auc_" + name] = float(learning.predictor_performance(p, q)[2])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--shapes', nargs='*', default=["4:20", "5:18", "6:16"], help="k:log2(rows)")
    ap.add_argument('--bases-per-row-k4', type=int, default=500, help="bases per row of the first shape; the buffer is shared")
    ap.add_argument('--cross-validate', nargs=2, metavar=("PF", "NF"))
    ap.add_argument('--folds', type=int, default=20)
    ap.add_argument('--method', default='combo')
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    from phamers_amd import _lib
    ctx = _lib.get_context()
    shapes = [tuple(int(x) for x in s.split(":")) for s in args.shapes]
    if shapes:
        total = max(1 << r for _, r in shapes) * args.bases_per_row_k4
        rng = np.random.RandomState(0)
        bases = np.frombuffer(b"ATGC", dtype=np.uint8)[rng.randint(0, 4, total, dtype=np.uint8)]
        for k, log2_rows in shapes:
            print(json.dumps(fold_shape(ctx, bases, k, log2_rows, args.repeat)), flush=True)
    if args.cross_validate:
        print(json.dumps(cross_validation_auc(args.cross_validate[0], args.cross_validate[1], args.folds, args.method, args.seed)),
              flush=True)


if __name__ == '__main__':
    main()
