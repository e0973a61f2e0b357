#!/usr/bin/env python3
"""
gen_golden_svm.py -- the parity fixture of the svm and dbscan scoring methods, tests/golden/scoring_svm.npz, produced by
running the REFERENCE's own phamer_scorer.svm_score_points (scripts/phamer.py:258-266) and dbscan_score_points
(scripts/phamer.py:212-238) with scikit-learn, through tools/gen_golden.py's ``extract`` (no reference text is stored).

The NuSVC each svm run fits is recorded through a thin subclass handed to the reference as its ``svm`` module, so the
stored support_, dual_coef_, intercept_, n_iter_ and gamma are those of the very fit that produced the scores.  Inputs
are taken from the fixtures that already hold them (ref_features.npz, scoring_k4.npz, scoring_highdim.npz); only a few
mixed query rows are new.  A query whose decision value is within 1e-5 of zero is refused: its predicted class would
hang on the last bits of the arithmetic.

Usage:  python tools/gen_golden_svm.py --ref <PhaMers checkout> [--out tests/golden]
"""
import argparse
import logging
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
from gen_golden import extract  # noqa: E402

CV_SEED, CV_N, CV_FOLDS = 7, 5, (0, 1)
DBSCAN_EPS = (0.02, 0.03)        # 0.02: DBSCAN clusters both classes; 0.03: the negative class falls back to k-means
MIN_MARGIN = 1e-5


def load_reference(ref, fits, svc_kw=None):
    import sklearn
    from sklearn.cluster import DBSCAN, KMeans
    from sklearn.svm import NuSVC

    class RecordingNuSVC(NuSVC):
        def __init__(self):
            super().__init__(**(svc_kw or {}))

        def fit(self, X, y, sample_weight=None):
            fits.append(self)
            return super().fit(X, y, sample_weight)

    scripts = os.path.join(ref, 'scripts')
    quiet = logging.getLogger('reference')
    quiet.setLevel(logging.ERROR)
    kmer = extract(os.path.join(scripts, 'kmer.py'), ['normalize_counts'], {'np': np, 'xrange': range, 'logger': quiet})
    learning = extract(os.path.join(scripts, 'learning.py'),
                       ['kmeans_seed', 'distances', 'closest_to', 'get_centroids', 'kmeans', 'dbscan'],
                       {'np': np, 'xrange': range, 'logger': quiet, 'KMeans': KMeans, 'DBSCAN': DBSCAN})
    ph_ns = {'np': np, 'xrange': range, 'logger': quiet, 'os': os, 'kmer': kmer, 'learning': learning,
             'svm': types.SimpleNamespace(NuSVC=RecordingNuSVC), '__file__': os.path.join(scripts, 'phamer.py')}
    phamer = extract(os.path.join(scripts, 'phamer.py'), ['phamer_scorer', 'score_points'], ph_ns)
    return kmer, learning, phamer, sklearn.__version__


def mixed_rows(pos, neg, n, seed):
    """Synthetic profiles: convex mixtures of a random positive and a random negative row, then a multinomial draw of
    4 997 4-mers (one 5 kb contig) from the mixture."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        w = rng.uniform(0.2, 0.8)
        p = w * pos[rng.randint(len(pos))] + (1 - w) * neg[rng.randint(len(neg))]
        c = rng.multinomial(4997, p / p.sum())
        out.append(c / float(c.sum()))
    return np.array(out)


def svm_case(ref, tag, q, pos, neg, svc_kw=None):
    fits = []
    phamer = load_reference(ref, fits, svc_kw)[2]
    pred = np.asarray(phamer.score_points(q, pos, neg, method='svm'), dtype=np.float64)
    (m,) = fits
    dec = m.decision_function(q)
    small = np.flatnonzero(np.abs(dec) < MIN_MARGIN)
    if len(small):
        raise SystemExit("case %s: queries %s have |decision| < %g" % (tag, small.tolist(), MIN_MARGIN))
    print("%-6s n_iter %d, %d support vectors, gamma %.6g, min |dec| %.3g" %
          (tag, m.n_iter_[0], len(m.support_), m._gamma, np.abs(dec).min()))
    return {'pred_' + tag: pred, 'dec_' + tag: dec, 'support_' + tag: m.support_.astype(np.int32),
            'dual_coef_' + tag: m.dual_coef_[0], 'intercept_' + tag: m.intercept_, 'n_iter_' + tag: m.n_iter_,
            'gamma_' + tag: np.array(m._gamma)}


def dbscan_case(phamer, learning, tag, q, pos, neg, eps):
    sc = phamer.phamer_scorer()
    sc.scoring_method = 'dbscan'
    if eps is not None:
        sc.eps = [eps, eps]
    sc.data_points, sc.positive_data, sc.negative_data = q, pos, neg
    scores = np.asarray(sc.score_points(), dtype=np.float64)
    arrays = {'dbscan_' + tag: scores, 'dbscan_eps_' + tag: np.array(sc.eps, dtype=np.float64)}
    for cls, data, e, ms, k in (('pos', pos, sc.eps[0], sc.min_samples[0], sc.k_clusters_positive),
                                ('neg', neg, sc.eps[1], sc.min_samples[1], sc.k_clusters_negative)):
        a = np.asarray(learning.dbscan(data, e, ms))
        arrays['dbscan_%s_labels_%s' % (cls, tag)] = a.astype(np.int16)
        if max(a) < 2:
            arrays['dbscan_%s_kmeans_%s' % (cls, tag)] = np.asarray(learning.kmeans(data, k)).astype(np.int16)
        print("dbscan %-5s %s: %d clusters, %d noise%s" % (tag, cls, a.max() + 1, (a == -1).sum(),
                                                          ", k-means fallback" if max(a) < 2 else ""))
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='a checkout of the reference (jondeaton/PhaMers)')
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    kmer, learning, phamer, skl = load_reference(args.ref, [])
    with np.load(os.path.join(args.out, 'ref_features.npz')) as z:
        pos = kmer.normalize_counts(z['pos_counts'].astype(np.int64))
        neg = kmer.normalize_counts(z['neg_counts'].astype(np.int64))
    with np.load(os.path.join(args.out, 'scoring_k4.npz')) as z:
        q4 = z['q']
    mix = mixed_rows(pos, neg, 28, 11)
    q = np.vstack((q4, mix))
    m = min(len(pos), len(neg))
    arrays = {'sklearn_version': np.array(skl), 'mix_q': mix, 'n_equalized': np.array([m, m])}
    # queries of the full / eq / auto cases: vstack(scoring_k4.npz q, mix_q)
    arrays.update(svm_case(args.ref, 'full', q, pos, neg))
    arrays.update(svm_case(args.ref, 'eq', q, pos[:m], neg[:m]))
    arrays.update(svm_case(args.ref, 'auto', q, pos[:m], neg[:m], {'gamma': 'auto'}))
    # cross-validation folds: the assignment of scripts/cross_validate.py:71-75 (N = 5, global RNG seeded), full
    # matrices; a fold trains on the other folds' rows and scores its own held-out rows, positive then negative
    np.random.seed(CV_SEED)
    pa = np.arange(len(pos)) % CV_N
    na = np.arange(len(neg)) % CV_N
    np.random.shuffle(pa)
    np.random.shuffle(na)
    arrays['cv_pos_asmt'], arrays['cv_neg_asmt'] = pa.astype(np.int16), na.astype(np.int16)
    for f in CV_FOLDS:
        qf = np.vstack((pos[pa == f], neg[na == f]))
        arrays.update(svm_case(args.ref, 'fold%d' % f, qf, pos[pa != f], neg[na != f]))
    with np.load(os.path.join(args.out, 'scoring_highdim.npz')) as z:
        arrays.update(svm_case(args.ref, 'k5', z['q_k5'], z['pos_k5'], z['neg_k5']))
    # dbscan: the reference's eps = [1, 1] (one cluster per class: both fall back to k-means 86 / 20), then smaller eps
    arrays.update(dbscan_case(phamer, learning, 'default', q4, pos, neg, None))
    for i, e in enumerate(DBSCAN_EPS):
        arrays.update(dbscan_case(phamer, learning, 'eps%d' % i, q4, pos, neg, e))
    path = os.path.join(args.out, 'scoring_svm.npz')
    np.savez_compressed(path, **arrays)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
