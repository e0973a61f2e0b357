#!/usr/bin/env python3
"""
gen_golden_density_sweep.py -- the scikit-learn fixture of the density bandwidth sweep, tests/golden/density_sweep.npz:
KernelDensity(kernel='gaussian', bandwidth=h).fit(X).score_samples(Q) for 64 queries x 200 rows x 3 bandwidths, and the
leave-one-out log-density of 40 rows (row i scored under a fit on the other 39), each computed with scikit-learn's KD tree
and once more with its ball tree: the trees' own sums are off by up to ~1e-9 on some rows (tools/gen_golden_density.py), so
the tests hold scikit-learn's values only where the two trees agree to 1e-10.  The scikit-learn version is recorded inside.

Usage:  python tools/gen_golden_density_sweep.py [--out tests/golden]
"""
import argparse
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDWIDTHS = (0.004, 0.01, 0.05)
N_QUERIES, N_ROWS, N_LOO, D = 64, 200, 40, 32


def rows(rng, n, base):
    """Normalised rows (row sum 1) a few hundredths apart, like normalised k-mer counts (much farther apart and the trees' own sums
    are off by tens of nats at the narrow bandwidths)."""
    x = base[None, :] * (1.0 + 0.1 * rng.standard_normal((n, len(base)))).clip(0.05)
    return x / x.sum(axis=1, keepdims=True)


def main():
    import sklearn
    from sklearn.neighbors import KernelDensity
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    rng = np.random.default_rng(20)
    base = rng.random(D) + 0.5
    X, Q = rows(rng, N_ROWS, base), rows(rng, N_QUERIES, base)
    Q[0] = X[7]                       # an exact duplicate of a data row
    Q[1] = 0.5 * (X[10] + X[11])      # equidistant from two rows
    arrays = {'sklearn_version': np.array(sklearn.__version__), 'X': X, 'Q': Q, 'bandwidths': np.array(BANDWIDTHS)}
    for tree in ('kd_tree', 'ball_tree'):
        sweep, loo = np.empty((len(BANDWIDTHS), N_QUERIES)), np.empty((len(BANDWIDTHS), N_LOO))
        for b, h in enumerate(BANDWIDTHS):
            sweep[b] = KernelDensity(kernel='gaussian', bandwidth=h, algorithm=tree).fit(X).score_samples(Q)
            for i in range(N_LOO):
                kde = KernelDensity(kernel='gaussian', bandwidth=h, algorithm=tree).fit(np.delete(X[:N_LOO], i, axis=0))
                loo[b, i] = kde.score_samples(X[i:i + 1])[0]
        arrays['sweep_' + tree], arrays['loo_' + tree] = sweep, loo
    path = os.path.join(args.out, 'density_sweep.npz')
    np.savez_compressed(path, **arrays)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
