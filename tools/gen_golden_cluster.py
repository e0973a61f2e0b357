#!/usr/bin/env python3
"""
gen_golden_cluster.py -- the parity fixture of the clustering analysis, tests/golden/clustering.npz, produced by running the
REFERENCE's own learning.dbscan, silhouettes, cluster_silhouettes, cluster_deviations, sort_assignment_by_size and kmeans
(scripts/learning.py) with the installed scikit-learn, through tools/gen_golden.py's ``extract`` (no reference text is
stored).  DBSCAN's core_sample_indices_ come from the same scikit-learn DBSCAN fit.

Inputs: the normalised rows of ref_features.npz (not stored again) and a few small synthetic sets (stored).  Every DBSCAN
case on the reference rows keeps all pair distances at least MIN_MARGIN away from eps (the margin is stored); the dyadic
set is the one deliberate exception: a pair at exactly eps.  The scikit-learn version is recorded inside the npz.

Usage:  python tools/gen_golden_cluster.py --ref <PhaMers checkout> [--out tests/golden]
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
from tests import cluster_ref  # noqa: E402  (direct-difference margins, the border-tie set)

DBSCAN_CASES = ((0.005, 2), (0.01, 2), (0.01, 5), (0.02, 3), (1.0, 2))
# Silhouettes of the DBSCAN labels of this case (noise included).  Not the smaller eps: their clusters hold near-duplicate
# rows, where scikit-learn's distances sqrt(|x|^2 + |y|^2 - 2 x.y) are the square root of rounding noise, and its
# silhouettes of a few positive rows are off by up to 1.2e-7 from the float64 direct-difference values (case 3: 1.1e-9).
SIL_DBSCAN_CASE = 3
K_CLUSTERS = 86
MIN_MARGIN = 1e-9


def load_reference(ref):
    import sklearn
    from sklearn.cluster import DBSCAN, KMeans
    from sklearn.metrics import silhouette_samples, silhouette_score
    scripts = os.path.join(ref, 'scripts')
    quiet = logging.getLogger('reference')
    quiet.setLevel(logging.ERROR)
    kmer = extract(os.path.join(scripts, 'kmer.py'), ['normalize_counts'], {'np': np, 'xrange': range, 'logger': quiet})
    ns = {'np': np, 'xrange': range, 'logger': quiet, 'DBSCAN': DBSCAN, 'KMeans': KMeans,
          'silhouette_samples': silhouette_samples, 'silhouette_score': silhouette_score}
    learning = extract(os.path.join(scripts, 'learning.py'),
                       ['kmeans_seed', 'dbscan', 'silhouettes', 'cluster_silhouettes', 'cluster_deviations',
                        'sort_assignment_by_size', 'get_centroids', 'distances', 'kmeans'], ns)
    return kmer, learning, sklearn.__version__


def blobs_2d():
    """Four 2-D blobs of 60 points and 12 scattered points (scikit-learn takes a KD tree at D = 2)."""
    rng = np.random.RandomState(3)
    centres = np.array([[0.0, 0.0], [4.0, 0.5], [1.0, 5.0], [6.0, 6.0]])
    X = np.vstack([c + 0.45 * rng.randn(60, 2) for c in centres] + [rng.uniform(-2, 8, (12, 2))])
    return X[rng.permutation(X.shape[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='a checkout of the reference (jondeaton/PhaMers)')
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    from sklearn.cluster import DBSCAN
    from sklearn.metrics import silhouette_score
    kmer, learning, skl = load_reference(args.ref)
    with np.load(os.path.join(args.out, 'ref_features.npz')) as z:
        classes = {'pos': kmer.normalize_counts(z['pos_counts'].astype(np.int64)),
                   'neg': kmer.normalize_counts(z['neg_counts'].astype(np.int64))}
    arrays = {'sklearn_version': np.array(skl), 'dbscan_cases': np.array(DBSCAN_CASES),
              'sil_dbscan_case': np.array([SIL_DBSCAN_CASE]), 'k_clusters': np.array([K_CLUSTERS])}

    def dbscan_case(tag, X, eps, ms, check_margin=True):
        labels = np.asarray(learning.dbscan(X, eps, ms))
        fit = DBSCAN(eps=eps, min_samples=ms).fit(X)
        assert np.array_equal(labels, fit.labels_)
        margin = cluster_ref.eps_margin(X, eps)
        if check_margin and margin < MIN_MARGIN:
            raise SystemExit('%s: a pair lies %.3g from eps = %g: refused' % (tag, margin, eps))
        arrays[tag + '_labels'] = labels.astype(np.int32)
        arrays[tag + '_core'] = fit.core_sample_indices_.astype(np.int32)
        arrays[tag + '_margin'] = np.array([margin])
        return labels

    for c, X in classes.items():
        for i, (eps, ms) in enumerate(DBSCAN_CASES):
            lab = dbscan_case('dbscan_%s_%d' % (c, i), X, eps, ms)
            print('%s eps=%g min_samples=%d: %d clusters, %d noise' % (c, eps, ms, len(set(lab) - {-1}), np.sum(lab == -1)))
            arrays['sorted_dbscan_%s_%d' % (c, i)] = learning.sort_assignment_by_size(lab, ascending=False).astype(np.int32)
        km = np.asarray(learning.kmeans(X, K_CLUSTERS)).astype(np.int32)
        arrays['kmeans_%s' % c] = km
        arrays['sil_kmeans_%s' % c] = np.asarray(learning.silhouettes(X, km))
        arrays['score_kmeans_%s' % c] = np.array([silhouette_score(X, km)])
        arrays['dev_kmeans_%s' % c] = np.asarray(learning.cluster_deviations(X, km))
        arrays['sorted_kmeans_%s_asc' % c] = learning.sort_assignment_by_size(km).astype(np.int32)
        arrays['sorted_kmeans_%s_desc' % c] = learning.sort_assignment_by_size(km, ascending=False).astype(np.int32)
        arrays['csil_kmeans_%s' % c] = np.asarray(learning.cluster_silhouettes(X, km, 0))
        dl = arrays['dbscan_%s_%d_labels' % (c, SIL_DBSCAN_CASE)]
        arrays['sil_dbscan_%s' % c] = np.asarray(learning.silhouettes(X, dl))
        arrays['csil_dbscan_%s_noise' % c] = np.asarray(learning.cluster_silhouettes(X, dl, -1))
        arrays['dev_dbscan_%s' % c] = np.asarray(learning.cluster_deviations(X, dl))

    # synthetic sets
    X = blobs_2d()
    arrays['blobs'] = X
    dbscan_case('dbscan_blobs', X, 0.6, 5)
    dbscan_case('dbscan_blobs_ms1', X, 0.3, 1)
    dbscan_case('dbscan_blobs_noise', X, 0.6, X.shape[0] + 1)
    for order in ('apb', 'bpa', 'pba'):
        dbscan_case('dbscan_tie_' + order, cluster_ref.border_tie(order), 0.9, 4)
    arrays['dyadic'] = np.array([[0.0, 0.0], [3.0, 4.0], [6.0, 8.0]])
    dbscan_case('dbscan_dyadic', arrays['dyadic'], 5.0, 2, check_margin=False)
    rng = np.random.RandomState(5)
    lab = np.array([-1, 3, 7])[rng.randint(0, 3, X.shape[0])]
    arrays['blobs_sparse_labels'] = lab.astype(np.int32)
    arrays['sil_blobs_sparse'] = np.asarray(learning.silhouettes(X, lab))
    arrays['csil_blobs_sparse_7'] = np.asarray(learning.cluster_silhouettes(X, lab, 7))
    single = rng.randint(0, 4, X.shape[0])
    single[[5, 17, 40]] = [10, 11, 12]                 # three singleton clusters
    arrays['blobs_single_labels'] = single.astype(np.int32)
    arrays['sil_blobs_single'] = np.asarray(learning.silhouettes(X, single))

    path = os.path.join(args.out, 'clustering.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
