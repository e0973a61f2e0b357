#!/usr/bin/env python
"""Times the paired ROC-area comparison (phamers_amd/compare.py -> phk_compare_*) against the NumPy / Python-integer
statement of the same computation (tests/compare_ref.py) on the host (profiles/compare/README.md).  The statement is the
comparison: the project had no such function before.  No ratio is fixed in advance.

The cells are the combo grid's: 2 255 + 2 418 rows of tests/golden/ref_features.npz, 20 folds, seed 0, k_neighbors x
k_clusters = 6 x 8 = 48 cells (one untimed ``combo_grid.sweep``), so C = 48, n = 4 673; B = 2 000 resamples, seed 0.

  check  before any figure: every column of ``compare.cells`` against the statement (placements by the P x N comparison,
         the bootstrap by the run formula, which tests/test_compare_host.py ties to the brute force)
  a      ``compare.cells`` (upload, 48 sorts, placements, Grams, 2 000 resamples, rationals, quantiles): after one untimed
         call, --repeats timed calls; the statement once
  b      where the device call goes: create / placements + Grams / bootstrap / host arithmetic, and the kernels of one
         profiled call (the context's event timers, a run of its own)
  c      the README's rows: (3, 86) against (1, 200), (1, 160) against (1, 200)

Reads nothing outside the repository.  One JSON line per figure.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K_NEIGHBORS = (1, 3, 5, 7, 9, 15)
K_CLUSTERS = (10, 20, 40, 60, 86, 120, 160, 200)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--resamples', type=int, default=2000)
    ap.add_argument('--folds', type=int, default=20)
    args = ap.parse_args()
    from statistics import NormalDist

    from phamers_amd import _lib, combo_grid, compare, kmer
    from tests import compare_ref
    ctx = _lib.get_context()
    with np.load(os.path.join(REPO, 'tests', 'golden', 'ref_features.npz')) as z:
        pos = kmer.normalize_counts(z['pos_counts'].astype(np.int64))
        neg = kmer.normalize_counts(z['neg_counts'].astype(np.int64))
    sweep = combo_grid.sweep(pos, neg, K_NEIGHBORS, K_CLUSTERS, args.folds, seed=0)
    m, P = compare.combo_cells(sweep), len(pos)
    C, n, B = m.shape[0], m.shape[1], args.resamples
    pairs = [(kn, kc) for kn in K_NEIGHBORS for kc in K_CLUSTERS]
    base = pairs.index((3, 86))

    def device():
        return compare.cells(m, P, baseline=base, resamples=B, seed=0)

    device()
    t_d = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        table = device()
        t_d.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = compare_ref.cells(m, P, baseline=base, resamples=B, seed=0, brute=False)
    t_h = time.perf_counter() - t0
    equal = {name: bool(np.array_equal(table[name], want[name], equal_nan=True)) for name in compare.COLUMNS}
    print(json.dumps({"case": "check", "cells": C, "rows": n, "resamples": B, "columns_equal": equal, "all_equal": all(equal.values())}))
    ms = lambda ts: [round(t * 1e3, 1) for t in ts]   # noqa: E731
    print(json.dumps({"case": "a", "device_ms": round(float(np.median(t_d)) * 1e3, 1), "device_runs": ms(t_d),
                      "device_spread_ms": round((max(t_d) - min(t_d)) * 1e3, 1), "host_statement_ms": round(t_h * 1e3, 1),
                      "host_runs": 1, "host_over_device": round(t_h / float(np.median(t_d)), 1)}))

    stages = {"create": [], "placements_grams": [], "bootstrap": [], "host_arithmetic": []}
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        c = compare.Comparison(m, P)
        t1 = time.perf_counter()
        t_pos, t_neg = c._h.placements()
        area2, g10, g01 = c._h.grams()
        t2 = time.perf_counter()
        b = c.bootstrap(B, seed=0)
        t3 = time.perf_counter()
        d = compare.DeLong(P, n - P, area2, t_pos, t_neg, g10, g01)
        d.against(base), d.interval(), b.interval(), [b.delta_interval(k, base) for k in range(C)]
        t4 = time.perf_counter()
        c.close()
        for name, t in zip(("create", "placements_grams", "bootstrap", "host_arithmetic"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            stages[name].append(t)
    print(json.dumps({"case": "b", "stage_ms": {name: ms(ts) for name, ts in stages.items()}}))
    ctx.profile_enable(True)
    ctx.profile_reset()
    device()
    ctx.sync()
    prof = ctx.profile()
    ctx.profile_enable(False)
    print(json.dumps({"case": "b", "kernels": {name: [round(t, 3), int(cnt)] for name, (t, cnt) in sorted(prof.items())}}))

    with compare.Comparison(m, P) as c:
        d, b = c.delong(), c.bootstrap(B, seed=0)
    q = NormalDist().inv_cdf(0.975)
    for a_cell, b_cell in (((1, 200), (3, 86)), ((1, 200), (1, 160)), ((3, 120), (3, 86))):
        ia, ib = pairs.index(a_cell), pairs.index(b_cell)
        delta, se = d.delta(ia, ib), float(np.sqrt(d.delta_variance(ia, ib)))
        lo, hi = b.delta_interval(ia, ib)
        print(json.dumps({"case": "c", "cell": list(a_cell), "against": list(b_cell), "auc": float(d.auc[ia]), "auc_against": float(d.auc[ib]),
                          "se": float(d.se[ia]), "se_against": float(d.se[ib]),
                          "correlation": float(d.covariance[ia, ib] / (d.se[ia] * d.se[ib])), "delta": delta, "delta_se": se,
                          "delong_low": delta - q * se, "delong_high": delta + q * se, "z": d.z(ia, ib), "p": d.p_value(ia, ib),
                          "boot_low": lo, "boot_high": hi}))


if __name__ == '__main__':
    main()
