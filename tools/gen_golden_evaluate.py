#!/usr/bin/env python3
"""
gen_golden_evaluate.py -- the parity fixture of the score evaluation, tests/golden/evaluation.npz: scikit-learn's roc_curve
and auc, and the REFERENCE's own predictor_performance, get_truth_table and get_predictor_metrics (scripts/learning.py:
185-243, through tools/gen_golden.py's ``extract``; no reference text is stored) on the seeded cases of
tests/evaluate_ref.py and on the score vectors of tests/golden/cross_validation.npz, plus the report texts of those
(scripts/cross_validate.py:174-192 for scores.txt; metrics.txt by the rule of cross_validator.make_metrics_file).

Usage:  python tools/gen_golden_evaluate.py --ref <PhaMers checkout> [--out tests/golden]
"""
import argparse
import os
import sys
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
from gen_golden import extract  # noqa: E402
from tests import evaluate_ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='a checkout of the reference (jondeaton/PhaMers)')
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    import pandas as pd
    import sklearn
    from sklearn.metrics import auc, roc_curve
    learning = extract(os.path.join(args.ref, 'scripts', 'learning.py'),
                       ['predictor_performance', 'get_truth_table', 'get_predictor_metrics'],
                       {'np': np, 'pd': pd, 'roc_curve': roc_curve, 'auc': auc})
    out = {'sklearn_version': np.array(sklearn.__version__)}

    def evaluate(tag, pos, neg):
        fpr, tpr, area = learning.predictor_performance(pos, neg)
        truth, scores = np.r_[np.ones(len(pos)), np.zeros(len(neg))].astype(bool), np.r_[pos, neg]
        for drop in (True, False):
            f, t, th = roc_curve(truth, scores, drop_intermediate=drop)
            if drop:
                assert np.array_equal(f, fpr) and np.array_equal(t, tpr)
            sfx = '' if drop else '_all'
            out['%s_fpr%s' % (tag, sfx)], out['%s_tpr%s' % (tag, sfx)], out['%s_thr%s' % (tag, sfx)] = f, t, th
        out[tag + '_auc'] = np.float64(area)
        ths = evaluate_ref.case_thresholds(pos, neg)
        out[tag + '_thresholds'] = np.array(ths)
        out[tag + '_truth'] = np.array([learning.get_truth_table(pos, neg, threshold=th) for th in ths], dtype=np.float64)
        with warnings.catch_warnings(), np.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            out[tag + '_metrics'] = np.array([[float(v) for v in learning.get_predictor_metrics(pos, neg, threshold=th).values]
                                              for th in ths], dtype=np.float64)   # NaN / inf where a denominator is zero

    for name, (pos, neg) in evaluate_ref.cases().items():
        evaluate(name, pos, neg)
    with np.load(os.path.join(args.out, 'cross_validation.npz')) as z:
        for tag in ('n7_knn', 'n20_combo'):
            pos, neg = z['pos_scores_' + tag], z['neg_scores_' + tag]
            evaluate('cv_' + tag, pos, neg)
            ids = ['p%04d' % i for i in range(len(pos))]     # (ascending as strings: tied scores keep this order)
            text = "# Cross Validation Scores"
            sorted_scores = sorted(pos)
            sorted_ids = [id for (score, id) in sorted(zip(pos, ids))]
            for i in range(len(sorted_ids)):
                text += "\n{id}\t{score}".format(id=sorted_ids[i], score=sorted_scores[i])
            out['cv_%s_summary' % tag] = np.array(text)
            m = learning.get_predictor_metrics(pos, neg, threshold=0)
            out['cv_%s_metrics_text' % tag] = np.array("# Cross Validation Performance Metrics\n" + "".join(
                "%s\t%r\n" % (name, float(m[name])) for name in evaluate_ref.METRIC_NAMES))
    np.savez_compressed(os.path.join(args.out, 'evaluation.npz'), **out)
    print("wrote evaluation.npz: %d arrays, scikit-learn %s" % (len(out), sklearn.__version__))


if __name__ == '__main__':
    main()
