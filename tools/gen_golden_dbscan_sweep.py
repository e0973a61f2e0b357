#!/usr/bin/env python3
"""
gen_golden_dbscan_sweep.py -- the parity fixture of the DBSCAN parameter sweep, tests/golden/dbscan_sweep.npz: scikit-learn's
``DBSCAN(eps, min_samples).fit(X).labels_`` for every cell of an eps x min_samples grid on the normalised phage rows of
ref_features.npz (not stored again), with the summary numbers of every cell.  Host only: no GPU is needed.

Every eps keeps all pair distances (float64 direct differences) at least MIN_MARGIN away from it, or the tool refuses; the
smallest |d_ij - eps| per eps and the scikit-learn version are stored.  (eps = 0.03 has a pair 2.5e-10 away and is not in
the grid for that reason.)  The fixture holds only data.

Usage:  python tools/gen_golden_dbscan_sweep.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import oracle  # noqa: E402
from tests import cluster_ref, dbscan_sweep_ref  # noqa: E402

EPS_VALUES = (0.004, 0.006, 0.008, 0.010, 0.012, 0.015, 0.020)
MIN_SAMPLES_VALUES = (2, 3, 5, 10)
MIN_MARGIN = 1e-9


def eps_margins(X, eps_values):
    """min |d_ij - eps| over all pairs i < j, for every eps, from one pass over the pairs."""
    margins = np.full(len(eps_values), np.inf)
    for s in range(0, X.shape[0], 256):
        d = cluster_ref.pair_distances(X[s:s + 256], X)
        upper = np.arange(s, min(s + 256, X.shape[0]))[:, None] < np.arange(X.shape[0])[None, :]
        for k, eps in enumerate(eps_values):
            margins[k] = min(margins[k], float(np.abs(d[upper] - eps).min()))
    return margins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    import sklearn
    from sklearn.cluster import DBSCAN
    with np.load(os.path.join(args.out, 'ref_features.npz')) as z:
        X = oracle.normalize_counts(z['pos_counts'].astype(np.int64))
    margins = eps_margins(X, EPS_VALUES)
    for eps, margin in zip(EPS_VALUES, margins):
        if margin < MIN_MARGIN:
            raise SystemExit('a pair lies %.3g from eps = %g: refused' % (margin, eps))
    labels, summary = [], {name: [] for name in dbscan_sweep_ref.SUMMARY}
    for eps in EPS_VALUES:
        for m in MIN_SAMPLES_VALUES:
            fit = DBSCAN(eps=eps, min_samples=m).fit(X)
            core = np.zeros(X.shape[0], dtype=bool)
            core[fit.core_sample_indices_] = True
            cell = dbscan_sweep_ref.summarize(fit.labels_, core)
            print('eps=%g min_samples=%d: %s' % (eps, m, cell))
            labels.append(fit.labels_.astype(np.int16))
            for name in dbscan_sweep_ref.SUMMARY:
                summary[name].append(cell[name])
    arrays = {'sklearn_version': np.array(sklearn.__version__), 'eps_values': np.array(EPS_VALUES, dtype=np.float64),
              'min_samples_values': np.array(MIN_SAMPLES_VALUES, dtype=np.int64), 'eps_margin': margins,
              'labels': np.stack(labels)}
    for name in dbscan_sweep_ref.SUMMARY:
        arrays[name] = np.array(summary[name], dtype=np.int64)
    path = os.path.join(args.out, 'dbscan_sweep.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
