"""
bandwidth.py -- the table behind a choice of the density method's two bandwidths (``phamer_scorer.positive_bandwidth`` /
``negative_bandwidth``, ``cross_validator``'s attributes of the same names): the held-out ROC area of L+(h+) - L-(h-) for
every cell of a grid h+ x h-, what dbscan_grid.py is to ``eps`` / ``min_samples`` and scripts/cluster.py to ``k_clusters``.

    held_out_log_densities(positive, negative, positive_bandwidths, negative_bandwidths, folds=None, seed=None)
                                    -> the four (bandwidth, row) arrays of held-out log-densities (learning.density_sweep)
    grid(...same arguments...)      -> one entry per cell, h+ outermost: positive_bandwidth, negative_bandwidth, auc
    python -m phamers_amd.bandwidth -data DIR | -pf FILE -nf FILE --positive_bandwidths V [V ...]
                                    --negative_bandwidths V [V ...] [-N FOLDS] [--seed S] [-out FILE]
                                    -> a CSV of positive_bandwidth, negative_bandwidth, auc

The reference fixes both bandwidths (scripts/phamer.py:82-83: 0.005 and 0.01) and has no such study.  A row's log-density
under its own class leaves the row out: by index with ``folds=None`` (leave-one-out), or with its fold of the validator's own
split (``cross_validate.FoldPlan``) with ``folds=N``.  The pair distances do not depend on the bandwidth, so every bandwidth
of an axis comes from one pass over the pairs.  The mean held-out log-likelihoods are reported, but
the ROC area is the criterion: on data with near-identical rows the likelihood keeps rising as the bandwidth shrinks.
Plots are out of scope: the table is written as a CSV.
"""
import argparse
import os

import numpy as np

from . import cross_validate, fileIO, learning

COLUMNS = ("positive_bandwidth", "negative_bandwidth", "auc")
ARRAYS = ("pos_under_pos", "neg_under_pos", "pos_under_neg", "neg_under_neg")


def _bandwidths(values, name):
    h = np.asarray(values, dtype=np.float64).ravel()
    if h.size == 0:
        raise ValueError("no %s bandwidths given" % name)
    if not (np.isfinite(h) & (h > 0)).all():
        raise ValueError("bandwidth must be finite and > 0, got %r" % (h.tolist(),))
    return h


def held_out_log_densities(positive, negative, positive_bandwidths, negative_bandwidths, folds=None, seed=None):
    """{``pos_under_pos`` (B+, n+), ``neg_under_pos`` (B+, n-), ``pos_under_neg`` (B-, n+), ``neg_under_neg`` (B-, n-)}:
    the log-density of every positive / negative row under the positive rows at each of ``positive_bandwidths`` and under
    the negative rows at each of ``negative_bandwidths``, the row itself held out of its own class.  ``folds=None``:
    leave-one-out, four ``learning.density_sweep`` calls (the same-class ones with ``exclude_self``).  ``folds=N``: the
    split of ``cross_validate.FoldPlan(n+, n-, N, seed)``; per fold the held-out rows are the queries and each class's
    train rows the data (four calls per fold)."""
    P = np.ascontiguousarray(positive, dtype=np.float64)
    Nm = np.ascontiguousarray(negative, dtype=np.float64)
    hp, hn = _bandwidths(positive_bandwidths, "positive"), _bandwidths(negative_bandwidths, "negative")
    if P.ndim != 2 or Nm.ndim != 2 or P.shape[1] != Nm.shape[1]:
        raise ValueError("positive and negative rows must be 2-D with the same number of columns")
    if np.isnan(P).any() or np.isnan(Nm).any():
        raise ValueError("Input contains NaN.")
    if folds is None:
        return {"pos_under_pos": learning.density_sweep(P, P, hp, exclude_self=True),
                "neg_under_pos": learning.density_sweep(Nm, P, hp),
                "pos_under_neg": learning.density_sweep(P, Nm, hn),
                "neg_under_neg": learning.density_sweep(Nm, Nm, hn, exclude_self=True)}
    plan = cross_validate.FoldPlan(len(P), len(Nm), folds, seed)
    out = {"pos_under_pos": np.empty((len(hp), len(P))), "neg_under_pos": np.empty((len(hp), len(Nm))),
           "pos_under_neg": np.empty((len(hn), len(P))), "neg_under_neg": np.empty((len(hn), len(Nm)))}
    for fold in range(plan.folds):
        out_p, out_n = plan.held_out(fold)
        train_p, train_n = P[~out_p], Nm[~out_n]
        out["pos_under_pos"][:, out_p] = learning.density_sweep(P[out_p], train_p, hp)
        out["neg_under_pos"][:, out_n] = learning.density_sweep(Nm[out_n], train_p, hp)
        out["pos_under_neg"][:, out_p] = learning.density_sweep(P[out_p], train_n, hn)
        out["neg_under_neg"][:, out_n] = learning.density_sweep(Nm[out_n], train_n, hn)
    return out


def grid(positive, negative, positive_bandwidths, negative_bandwidths, folds=None, seed=None):
    """The table as a dict of arrays, one entry per cell in the order ``for h+ in positive_bandwidths: for h- in
    negative_bandwidths`` (the values as given): ``positive_bandwidth``, ``negative_bandwidth`` and ``auc`` -- the ROC area
    ``learning.predictor_performance(pos_under_pos[a] - pos_under_neg[b], neg_under_pos[a] - neg_under_neg[b])[2]`` of the
    held-out scores -- beside ``loglik_positive`` (B+,) and ``loglik_negative`` (B-,), the mean held-out log-likelihood of
    each class under itself, and ``best``: the index of the cell of largest ``auc``, the first such cell on a tie."""
    L = held_out_log_densities(positive, negative, positive_bandwidths, negative_bandwidths, folds=folds, seed=seed)
    hp, hn = _bandwidths(positive_bandwidths, "positive"), _bandwidths(negative_bandwidths, "negative")
    auc = [learning.predictor_performance(L["pos_under_pos"][a] - L["pos_under_neg"][b],
                                          L["neg_under_pos"][a] - L["neg_under_neg"][b])[2]
           for a in range(len(hp)) for b in range(len(hn))]
    auc = np.array(auc, dtype=np.float64)
    return {"positive_bandwidth": np.repeat(hp, len(hn)), "negative_bandwidth": np.tile(hn, len(hp)), "auc": auc,
            "loglik_positive": L["pos_under_pos"].mean(axis=1), "loglik_negative": L["neg_under_neg"].mean(axis=1),
            "best": int(np.argmax(auc))}


def save_grid(filename, table, args=None):
    """One 'positive_bandwidth,negative_bandwidth,auc' row per cell (the floats as ``repr`` prints them) under a '# '
    comment header."""
    header = "Density bandwidth grid: " + ",".join(COLUMNS)
    if args is not None:
        header = fileIO.generate_summary(args, header=header).rstrip('\n')
    with open(filename, 'w') as f:
        f.write('# ' + header.replace('\n', '\n# ') + '\n')
        for i in range(len(table["auc"])):
            f.write('%r,%r,%r\n' % tuple(float(table[name][i]) for name in COLUMNS))


def read_grid(filename):
    """The per-cell arrays (and ``best``) of a file save_grid wrote."""
    rows = [line.strip().split(',') for line in open(filename) if not line.startswith('#') and line.strip()]
    out = {name: np.array([float(r[k]) for r in rows], dtype=np.float64) for k, name in enumerate(COLUMNS)}
    out["best"] = int(np.argmax(out["auc"])) if rows else None
    return out


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m phamers_amd.bandwidth", description=__doc__.split('\n\n')[0])
    parser.add_argument('-data', '--data_directory', help="Directory containing reference_features/")
    parser.add_argument('-pf', '--positive_features_file', help="Positive features file")
    parser.add_argument('-nf', '--negative_features_file', help="Negative features file")
    parser.add_argument('-out', '--output_file', help="Filename for the output CSV")
    parser.add_argument('--positive_bandwidths', nargs='+', type=float, required=True, help="the h+ values of the grid")
    parser.add_argument('--negative_bandwidths', nargs='+', type=float, required=True, help="the h- values of the grid")
    parser.add_argument('-N', '--N_fold', type=int, default=None,
                        help="Folds of the validator's split (leave-one-out when absent)")
    parser.add_argument('--seed', type=int, default=None, help="Seed of the fold assignment")
    args = parser.parse_args(argv)
    pf, nf = args.positive_features_file, args.negative_features_file
    if args.data_directory:
        ref = os.path.join(args.data_directory, "reference_features")
        pf, nf = pf or os.path.join(ref, "positive_features.csv"), nf or os.path.join(ref, "negative_features.csv")
    if not (pf and nf):
        parser.error("give -data DIR or both -pf FILE and -nf FILE")
    positive = fileIO.read_feature_file(pf, normalize=True)[1]
    negative = fileIO.read_feature_file(nf, normalize=True)[1]
    table = grid(positive, negative, args.positive_bandwidths, args.negative_bandwidths, folds=args.N_fold, seed=args.seed)
    save_grid(args.output_file or "density_bandwidths.csv", table, args=args)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
