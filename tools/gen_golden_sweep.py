#!/usr/bin/env python3
"""
gen_golden_sweep.py -- the parity fixture of the silhouette-against-k sweep, tests/golden/sweep.npz, produced by running the
REFERENCE's own code with the installed scikit-learn through tools/gen_golden.py's ``extract`` (no reference text is
stored): learning.kmeans and the silhouette_score scripts/cluster.py:43 calls through the learning module
(scripts/learning.py).  The reference keeps only the labels of a fit; its KMeans is wrapped here to record n_iter_ as well.

Cases: the 2255 normalised phage rows of ref_features.npz (not stored again) at k in PHAGE_K, random_state 10; two synthetic
sets of seeded Gaussian blobs plus noise (stored whole, as int16 multiples of 1/4096) at the k of SYNTH and random_state 10 and 11.  Per fit: labels
(int16), n_iter, the mean silhouette, and -- from the direct-difference restatement tests/sweep_ref.py -- the seeding margin
and the smallest assignment gap, which say whether the device may keep the problem.  A synthetic case is
refused, and the next data seed tried, when the restated seeding margin is below 1e-8, the restated gap below 1e-7, a
cluster ran empty, or the restatement's labels differ from scikit-learn's.

Usage:  python tools/gen_golden_sweep.py --ref <PhaMers checkout> [--out tests/golden]
"""
import argparse
import logging
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
from gen_golden import extract  # noqa: E402
from tests import sweep_ref  # noqa: E402

PHAGE_K = (10, 40, 86, 150, 300, 590)
SYNTH = (('s24', 300, 24, (2, 3, 5, 8, 13, 50, 299)), ('s130', 130, 130, (2, 7, 129)))   # name, rows, D, k values
SYNTH_SEEDS = (10, 11)
MIN_MARGIN, MIN_GAP = 1e-8, 1e-7
X_SCALE = 4096.0


def load_reference(ref):
    from sklearn.cluster import DBSCAN, KMeans
    from sklearn.metrics import silhouette_samples, silhouette_score
    scripts = os.path.join(ref, 'scripts')
    quiet = logging.getLogger('reference')
    quiet.setLevel(logging.ERROR)
    fits = []

    class RecordingKMeans(KMeans):
        def fit(self, X, y=None, sample_weight=None):
            out = KMeans.fit(self, X, y, sample_weight)
            fits.append(int(self.n_iter_))
            return out

    kmer = extract(os.path.join(scripts, 'kmer.py'), ['normalize_counts'], {'np': np, 'xrange': range, 'logger': quiet})
    ns = {'np': np, 'xrange': range, 'logger': quiet, 'DBSCAN': DBSCAN, 'KMeans': RecordingKMeans,
          'silhouette_samples': silhouette_samples, 'silhouette_score': silhouette_score}
    learning = extract(os.path.join(scripts, 'learning.py'), ['kmeans_seed', 'sort_assignment_by_size', 'kmeans'], ns)
    learning.silhouette_score = silhouette_score    # (a name scripts/learning.py imports; scripts/cluster.py:43 calls it there)
    return kmer, learning, fits


def fit(learning, fits, X, k, seed):
    """The reference's fit and score, and the restatement's guards."""
    learning.kmeans.__globals__['kmeans_seed'] = seed
    labels = np.asarray(learning.kmeans(X, k))
    sil = float(np.mean(learning.silhouette_score(X, labels)))        # scripts/cluster.py:43-44
    ref = sweep_ref.kmeans(X, k, seed)
    return {'labels': labels, 'n_iter': fits[-1], 'sil': sil, 'margin': ref['seed_margin'], 'gap': ref['min_gap'],
            'n_empty': ref['n_empty'], 'same': bool(np.array_equal(ref['labels'], labels) and ref['n_iter'] == fits[-1])}


def blobs(rows, D, seed):
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-1, 1, (6, D))
    X = centres[rng.randint(0, 6, rows)] + 0.25 * rng.randn(rows, D) + 0.05 * rng.uniform(-1, 1, (rows, D))
    return np.round(X * X_SCALE).astype(np.int16)   # stored as int16: the rows are these integers / X_SCALE, exactly


def pack(arrays, name, ks, seeds, results):
    arrays[name + '_k'] = np.array([k for k in ks for _ in seeds], dtype=np.int32)
    arrays[name + '_seed'] = np.array([s for _ in ks for s in seeds], dtype=np.int32)
    arrays[name + '_labels'] = np.array([r['labels'] for r in results]).astype(np.int16)
    arrays[name + '_n_iter'] = np.array([r['n_iter'] for r in results], dtype=np.int32)
    arrays[name + '_sil'] = np.array([r['sil'] for r in results], dtype=np.float64)
    arrays[name + '_margin'] = np.array([r['margin'] for r in results], dtype=np.float64)
    arrays[name + '_gap'] = np.array([r['gap'] for r in results], dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='a checkout of the reference (jondeaton/PhaMers)')
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    kmer, learning, fits = load_reference(args.ref)
    with np.load(os.path.join(args.out, 'ref_features.npz')) as z:
        pos = kmer.normalize_counts(z['pos_counts'].astype(np.int64))
    arrays = {}
    results = []
    for k in PHAGE_K:
        r = fit(learning, fits, pos, k, 10)
        singles = int(np.sum(np.bincount(r['labels'], minlength=k) == 1))
        print('phage k=%d sweeps %d silhouette %.6f margin %.3g gap %.3g empty %d restatement equal %s singletons %d'
              % (k, r['n_iter'], r['sil'], r['margin'], r['gap'], r['n_empty'], r['same'], singles))
        r['singles'] = singles
        results.append(r)
    pack(arrays, 'phage', PHAGE_K, (10,), results)
    arrays['phage_singletons'] = np.array([r['singles'] for r in results], dtype=np.int32)
    assert arrays['phage_singletons'][-2] > 0 and arrays['phage_singletons'][-1] > 0    # k = 300, 590 cover the singleton rule

    for name, rows, D, ks in SYNTH:
        data_seed = len(name) + D
        while True:
            Xq = blobs(rows, D, data_seed)
            X = Xq / X_SCALE
            results, why = [], None
            for k in ks:
                for seed in SYNTH_SEEDS:
                    r = fit(learning, fits, X, k, seed)
                    results.append(r)
                    if r['margin'] < MIN_MARGIN or r['gap'] < MIN_GAP or r['n_empty'] or not r['same']:
                        why = 'k=%d seed=%d margin %.3g gap %.3g empty %d equal %s' % (k, seed, r['margin'], r['gap'],
                                                                                      r['n_empty'], r['same'])
                        break
                if why:
                    break
            if why is None:
                break
            print('%s: data seed %d refused (%s)' % (name, data_seed, why))
            data_seed += 1
        for (k, seed), r in zip([(k, s) for k in ks for s in SYNTH_SEEDS], results):
            print('%s k=%d seed=%d sweeps %d silhouette %.6f margin %.3g gap %.3g' % (name, k, seed, r['n_iter'], r['sil'],
                                                                                    r['margin'], r['gap']))
        arrays[name + '_Xq'] = Xq
        arrays[name + '_scale'] = np.array([X_SCALE])
        arrays[name + '_data_seed'] = np.array([data_seed])
        pack(arrays, name, ks, SYNTH_SEEDS, results)

    path = os.path.join(args.out, 'sweep.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
