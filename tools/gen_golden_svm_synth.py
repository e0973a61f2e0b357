#!/usr/bin/env python3
"""
gen_golden_svm_synth.py -- tests/golden/scoring_svm_synth.npz: scikit-learn NuSVC fits on synthetic dyadic data, for the
paths of the GPU solver that the reference's data never reach (tests/test_svm_host.py, tests/test_gpu_svm.py).

Every feature is a multiple of 2^-12 (stored as int16 codes, x = code / 4096), so every norm, dot product and squared
distance is exact in float64 whatever the summation order: the GPU's MFMA Gram product and NumPy's give the same Q.

Cases (data set, NuSVC arguments):
    long      3 000 x 33, label x0 + x1 > 0.9 with 30 % flipped, nu = 0.5: about 10 000 iterations (three launches of
              the GPU solver).  Rows 0/1 are an exact duplicate with the same label, rows 2/3 one with opposite labels,
              and rows 8.. hold 50 near-duplicate pairs of each kind (one column apart by 2^-12: Q_ij rounds to 1.0f but
              the gradients differ), which take libsvm's TAU branches.
    maxiter   the long data with max_iter = 4097 (scikit-learn warns that it did not converge; the result is recorded).
    shrink    1 500 x 17 with entries k / 8, 45 % flipped, nu = 0.3: a case where NuSVC() (shrinking on) and
              NuSVC(shrinking=False) reach different solutions, and predict a few queries differently.
Each case is fitted twice, with shrinking off ("_noshrink") and scikit-learn's default ("_default"); the record holds
support_, dual_coef_, intercept_, n_iter_, _gamma, and decision values and predictions for the data set's queries.
A query is kept only if every fit of its data set puts it at least 1e-5 from the decision boundary.

Usage:  python tools/gen_golden_svm_synth.py [--out tests/golden]
"""
import argparse
import os
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_MARGIN = 1e-5
UNIT = 4096
NEAR_PAIRS = 50


def long_data():
    rng = np.random.default_rng(1)
    n, D = 3000, 33
    C = rng.integers(0, 8, (n, D)) * (UNIT // 8)
    lab = ((C[:, 0] + C[:, 1]) / UNIT > 0.9).astype(np.int64)
    lab[rng.random(n) < 0.3] ^= 1
    C[1], lab[1] = C[0], lab[0]                 # exact duplicate, same label
    C[3], lab[3] = C[2], 1 - lab[2]             # exact duplicate, opposite labels
    for k in range(8, 8 + 4 * NEAR_PAIRS, 4):   # near duplicates: d^2 = 2^-24
        C[k + 1], lab[k + 1] = C[k], lab[k]
        C[k + 1, k % D] += 1
        C[k + 3], lab[k + 3] = C[k + 2], 1 - lab[k + 2]
        C[k + 3, k % D] += 1
    q = rng.integers(0, 8, (500, D)) * (UNIT // 8)
    return C, lab, q


def shrink_data():
    rng = np.random.default_rng(5028)
    n, D = 1500, 17
    X = rng.integers(0, 8, (n, D))
    lab = ((X[:, 0] + X[:, 1]) / 8.0 > 0.9).astype(np.int64)
    lab[rng.random(n) < 0.45] ^= 1
    q = rng.integers(0, 8, (500, D))
    return X * (UNIT // 8), lab, q * (UNIT // 8)


def fit(X, lab, **kw):
    from sklearn.svm import NuSVC
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # max_iter: "Solver terminated early"
        return NuSVC(**kw).fit(X, lab)


def main():
    import sklearn
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden'))
    args = ap.parse_args()
    arrays = {'sklearn_version': np.array(sklearn.__version__), 'unit': np.array(UNIT)}
    data = {'long': long_data(), 'shrink': shrink_data()}
    cases = (('long', 'long', {}), ('maxiter', 'long', {'max_iter': 4097}), ('shrink', 'shrink', {'nu': 0.3}))
    for name, (C, lab, q) in data.items():
        arrays['X_' + name] = C.astype(np.int16)
        arrays['y_' + name] = lab.astype(np.int8)
    fits = {}
    for case, ds, kw in cases:
        C, lab, _ = data[ds]
        for mode, shrinking in (('noshrink', False), ('default', True)):
            fits[case, mode] = fit(C / float(UNIT), lab, shrinking=shrinking, **kw)
    for name, (C, lab, q) in data.items():
        Q = q / float(UNIT)
        keep = np.ones(len(q), dtype=bool)
        for (case, mode), m in fits.items():
            if dict((c, d) for c, d, _ in cases)[case] == name:
                keep &= np.abs(m.decision_function(Q)) >= MIN_MARGIN
        arrays['q_' + name] = q[keep].astype(np.int16)
        print("%-7s %d x %d, %d of %d queries kept" % (name, C.shape[0], C.shape[1], keep.sum(), len(q)))
    for (case, mode), m in fits.items():
        ds = dict((c, d) for c, d, _ in cases)[case]
        Q = arrays['q_' + ds] / float(UNIT)
        t = case + '_' + mode
        arrays.update({'support_' + t: m.support_.astype(np.int32), 'dual_coef_' + t: m.dual_coef_[0],
                       'intercept_' + t: m.intercept_, 'n_iter_' + t: m.n_iter_.astype(np.int32),
                       'gamma_' + t: np.array(m._gamma), 'dec_' + t: m.decision_function(Q),
                       'pred_' + t: m.predict(Q).astype(np.int8)})
        print("%-16s n_iter %d, %d support vectors, intercept %.17g" % (t, m.n_iter_[0], len(m.support_), m.intercept_[0]))
    for case, _, kw in cases:
        arrays['nu_' + case] = np.array(kw.get('nu', 0.5))
        arrays['max_iter_' + case] = np.array(kw.get('max_iter', -1))
    path = os.path.join(args.out, 'scoring_svm_synth.npz')
    np.savez_compressed(path, **arrays)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
