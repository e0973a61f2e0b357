#!/usr/bin/env python3
"""
gen_golden_density.py -- the parity fixture of the density scoring method, tests/golden/scoring_density.npz, produced by
running the REFERENCE's own phamer_scorer.density_score_points (scripts/phamer.py:275-287) and learning.get_density
(scripts/learning.py:107-115) with scikit-learn's KernelDensity, as tools/gen_golden.py does for the other methods (its
``extract`` helper: the wanted definitions are exec'd from the reference text; no reference text is stored).

Inputs are taken from the fixtures that already hold them (scoring_k4.npz: the query contigs; ref_features.npz: the
reference matrix; scoring_highdim.npz: the k = 5 / 6 sets) and are not stored again; only a few adversarial query rows
are new.  The scikit-learn version is recorded inside the npz.

Usage:  python tools/gen_golden_density.py --ref <PhaMers checkout> [--out tests/golden]
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

# bandwidth pairs beside the reference's (0.005, 0.01): wider kernels, and the two swapped
BANDWIDTH_PAIRS = ((0.02, 0.03), (0.01, 0.005))
CV_SEED, CV_N = 7, 5


def load_reference(ref, algorithm=None):
    """The reference's definitions; ``algorithm`` pins the tree KernelDensity builds (None: its default, 'auto')."""
    import sklearn
    from sklearn.neighbors import KernelDensity
    if algorithm is not None:
        tree_kde = KernelDensity

        def KernelDensity(**kw):   # noqa: N802 -- stands in for the class in the reference's namespace
            return tree_kde(algorithm=algorithm, **kw)
    scripts = os.path.join(ref, 'scripts')
    quiet = logging.getLogger('reference')
    quiet.setLevel(logging.ERROR)
    kmer = extract(os.path.join(scripts, 'kmer.py'), ['normalize_counts'], {'np': np, 'xrange': range, 'logger': quiet})
    learning = extract(os.path.join(scripts, 'learning.py'), ['get_density'],
                       {'np': np, 'xrange': range, 'logger': quiet, 'KernelDensity': KernelDensity})
    ph_ns = {'np': np, 'xrange': range, 'logger': quiet, 'os': os, 'kmer': kmer, 'learning': learning,
             '__file__': os.path.join(scripts, 'phamer.py')}
    phamer = extract(os.path.join(scripts, 'phamer.py'), ['phamer_scorer', 'score_points'], ph_ns)
    cv = extract(os.path.join(scripts, 'cross_validate.py'), ['cross_validator'],
                 {'np': np, 'xrange': range, 'logger': quiet})
    return kmer, learning, phamer, cv, sklearn.__version__


def density_scores(phamer, q, pos, neg, bandwidths=None):
    """phamer_scorer.density_score_points on q against (pos, neg), through the reference's score_points."""
    sc = phamer.phamer_scorer()
    sc.scoring_method = 'density'
    if bandwidths is not None:
        sc.positive_bandwidth, sc.negative_bandwidth = bandwidths
    sc.data_points, sc.positive_data, sc.negative_data = q, pos, neg
    return np.asarray(sc.score_points(), dtype=np.float64)


def adversarial_rows(pos, neg):
    """homopolymer profile (all windows one k-mer: d^2 ~ 1 from every row, exponents ~ -2e4), exact duplicates of a
    positive and a negative train row, the midpoint of two train rows (equidistant from both)."""
    homo = np.zeros(pos.shape[1])
    homo[0] = 1.0
    return np.vstack((homo, pos[3], neg[17], 0.5 * (pos[100] + pos[101]), 0.5 * (pos[5] + neg[5])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='a checkout of the reference (jondeaton/PhaMers)')
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    kmer, learning, phamer, cv, skl = load_reference(args.ref)
    with np.load(os.path.join(args.out, 'scoring_k4.npz')) as z:
        q = z['q']
    with np.load(os.path.join(args.out, 'ref_features.npz')) as z:
        pos = kmer.normalize_counts(z['pos_counts'].astype(np.int64))
        neg = kmer.normalize_counts(z['neg_counts'].astype(np.int64))
    adv = adversarial_rows(pos, neg)
    qa = np.vstack((q, adv))
    m = min(pos.shape[0], neg.shape[0])
    arrays = {'sklearn_version': np.array(skl), 'adv_q': adv, 'n_equalized': np.array([m, m]),
              'bandwidth_pairs': np.array(BANDWIDTH_PAIRS)}
    # queries = vstack(scoring_k4.npz q, adv_q)
    arrays['density_full'] = density_scores(phamer, qa, pos, neg)
    arrays['density_eq'] = density_scores(phamer, qa, pos[:m], neg[:m])
    for i, bw in enumerate(BANDWIDTH_PAIRS):
        arrays['density_full_bw%d' % i] = density_scores(phamer, q, pos, neg, bw)
    # learning.get_density at its default bandwidth (0.1), first 10 queries + the adversarial rows, per class
    pts = np.vstack((q[:10], adv))
    arrays['get_density_pos'] = np.array([learning.get_density(p, pos) for p in pts])
    arrays['get_density_neg'] = np.array([learning.get_density(p, neg) for p in pts])
    with np.load(os.path.join(args.out, 'scoring_highdim.npz')) as z:
        for k in (5, 6):
            t = 'k%d' % k
            arrays['density_' + t] = density_scores(phamer, z['q_' + t], z['pos_' + t], z['neg_' + t])
    # cross_validator.cross_validate (scripts/cross_validate.py:57-101), equalised, method 'density', seeded global RNG.
    # The reference's KernelDensity picks a KD tree here; on ~1 % of the held-out rows that tree's sum is off by up to ~10
    # nats (one row of fold 1: 1078.04 where the dense float64 sum gives 1068.29), and a ball tree is off on ~1 % of other
    # rows (both are off by ~1e-9 on a few more).  The run is stored as the reference made it, and once more with the ball
    # tree: rows where the two trees agree to 1e-10 (~97 %) are the ones the tests hold scikit-learn's values to.
    arrays.update(cross_validation(cv, phamer, pos, neg, ''))
    arrays.update(cross_validation(cv, load_reference(args.ref, 'ball_tree')[2], pos, neg, '_balltree'))
    path = os.path.join(args.out, 'scoring_density.npz')
    np.savez_compressed(path, **arrays)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def cross_validation(cv, phamer, pos, neg, suffix):
    arrays = {}
    v = cv.cross_validator()
    v.positive_data, v.negative_data = pos, neg
    v.positive_ids, v.negative_ids = np.arange(pos.shape[0]), np.arange(neg.shape[0])
    v.equalize_reference = True
    v.N = CV_N
    v.method = 'density'
    v.scoring_function = phamer.score_points
    np.random.seed(CV_SEED)
    ps, ns = v.cross_validate()
    np.random.seed(CV_SEED)    # the fold assignment, replayed (same draws as scripts/cross_validate.py:71-75)
    pa = np.arange(v.num_positive) % CV_N
    na = np.arange(v.num_negative) % CV_N
    np.random.shuffle(pa)
    np.random.shuffle(na)
    arrays['cv_pos_scores' + suffix], arrays['cv_neg_scores' + suffix] = np.asarray(ps), np.asarray(ns)
    if not suffix:
        arrays['cv_pos_asmt'], arrays['cv_neg_asmt'] = pa.astype(np.int16), na.astype(np.int16)
        arrays['cv_meta'] = np.array([CV_SEED, CV_N, v.num_positive, v.num_negative])
    return arrays


if __name__ == '__main__':
    main()
