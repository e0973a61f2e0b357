"""
svm_grid.py -- the table behind a choice of the svm method's two parameters (``phamer_scorer.svm_nu`` / ``svm_gamma``,
``cross_validator``'s attributes of the same names): the held-out ROC area and accuracy of NuSVC(nu, gamma) for every cell of a
grid gamma x nu, what bandwidth.py is to the density method's bandwidths and dbscan_grid.py to ``eps`` / ``min_samples``.

    grid(positive, negative, nus, gammas, folds, seed=None)
                                    -> one entry per cell, gamma outermost: gamma, nu, n_support, n_iter, auc, accuracy
    python -m phamers_amd.svm_grid -data DIR | -pf FILE -nf FILE --nu V [V ...] --gamma V [V ...] [--gamma_scale M [M ...]]
                                    -N FOLDS [--seed S] [-out FILE]
                                    -> a CSV of gamma, nu, n_support, n_iter, auc, accuracy

The reference fits ``svm.NuSVC()`` with scikit-learn's defaults (scripts/phamer.py:258-266: nu 0.5, gamma 'scale') and has no
such study.  A row is scored by the fit of the fold that held it out, in the validator's own split
(``cross_validate.FoldPlan``); every fit of the grid -- cells x (folds + 1) -- is solved side by side on the device
(``svm.nusvc_sweep``).  ``--gamma_scale`` gives multiples of 'scale' (1 / (D var(X)) over all rows);
the value is fixed for the whole table, while ``cross_validator`` with ``svm_gamma='scale'`` takes it over each fold's train
rows: set ``svm_gamma`` to the table's number to reproduce a cell.  ``n_support`` and ``n_iter`` are those of the fit on all
rows.  Plots are out of scope: the table is written as a CSV.
"""
import argparse
import os

import numpy as np

from . import _lib, fileIO, svm

COLUMNS = ("gamma", "nu", "n_support", "n_iter", "auc", "accuracy")


def grid(positive, negative, nus, gammas, folds, seed=None):
    """The table as a dict of arrays, one entry per cell in the order ``for gamma in gammas: for nu in nus``: ``gamma`` (as
    numbers: 'scale' / 'auto' resolved over all rows), ``nu``, ``n_support`` and ``n_iter`` of the fit on all rows, ``auc`` and
    ``accuracy`` of the held-out decisions (NaN for a cell with an infeasible or non-finite fit), ``status``, and ``best``:
    the index of the cell of largest ``auc``, the first such cell on a tie (None when every cell is NaN)."""
    P = np.ascontiguousarray(positive, dtype=np.float64)
    Nm = np.ascontiguousarray(negative, dtype=np.float64)
    if P.ndim != 2 or Nm.ndim != 2 or P.shape[1] != Nm.shape[1]:
        raise ValueError("positive and negative rows must be 2-D with the same number of columns")
    if folds is None or int(folds) < 2:
        raise ValueError("the table needs folds >= 2, got %r" % (folds,))
    X = np.vstack((P, Nm))
    y = np.r_[np.ones(len(P)), np.zeros(len(Nm))]
    res = svm.nusvc_sweep(X, y, nus, gammas, folds=folds, seed=seed)
    V = len(res.nus)
    auc = res.auc.ravel()
    return {"gamma": np.repeat(res.gammas, V), "nu": np.tile(res.nus, len(res.gammas)),
            "n_support": res.n_support.ravel().astype(np.float64), "n_iter": res.n_iter.ravel().astype(np.float64),
            "auc": auc, "accuracy": res.accuracy.ravel(), "status": res.status.ravel(),
            "best": None if np.isnan(auc).all() else int(np.nanargmax(auc))}


def save_grid(filename, table, args=None):
    """One 'gamma,nu,n_support,n_iter,auc,accuracy' row per cell (the floats as ``repr`` prints them, the counts as
    integers) under a '# ' comment header."""
    header = "NuSVC nu x gamma grid: " + ",".join(COLUMNS)
    if args is not None:
        header = fileIO.generate_summary(args, header=header).rstrip('\n')
    with open(filename, 'w') as f:
        f.write('# ' + header.replace('\n', '\n# ') + '\n')
        for i in range(len(table["auc"])):
            f.write('%r,%r,%d,%d,%r,%r\n' % (float(table["gamma"][i]), float(table["nu"][i]), int(table["n_support"][i]),
                                             int(table["n_iter"][i]), float(table["auc"][i]), float(table["accuracy"][i])))


def read_grid(filename):
    """The per-cell arrays (and ``best``) of a file save_grid wrote."""
    rows = [line.strip().split(',') for line in open(filename) if not line.startswith('#') and line.strip()]
    out = {name: np.array([float(r[k]) for r in rows], dtype=np.float64) for k, name in enumerate(COLUMNS)}
    out["best"] = None if not rows or np.isnan(out["auc"]).all() else int(np.nanargmax(out["auc"]))
    return out


def _parser():
    parser = argparse.ArgumentParser(prog="python -m phamers_amd.svm_grid", description=__doc__.split('\n\n')[0])
    parser.add_argument('-data', '--data_directory', help="Directory containing reference_features/")
    parser.add_argument('-pf', '--positive_features_file', help="Positive features file")
    parser.add_argument('-nf', '--negative_features_file', help="Negative features file")
    parser.add_argument('-out', '--output_file', help="Filename for the output CSV")
    parser.add_argument('--nu', nargs='+', type=float, required=True, help="the nu values of the grid")
    parser.add_argument('--gamma', nargs='+', type=float, default=[], help="the gamma values of the grid, as numbers")
    parser.add_argument('--gamma_scale', nargs='+', type=float, default=[],
                        help="further gamma values as multiples of 'scale' = 1 / (D var(X)) over all rows")
    parser.add_argument('-N', '--N_fold', type=int, required=True, help="Folds of the validator's split")
    parser.add_argument('--seed', type=int, default=None, help="Seed of the fold assignment")
    return parser


def main(argv=None):
    parser = _parser()
    args = parser.parse_args(argv)
    pf, nf = args.positive_features_file, args.negative_features_file
    if args.data_directory:
        ref = os.path.join(args.data_directory, "reference_features")
        pf, nf = pf or os.path.join(ref, "positive_features.csv"), nf or os.path.join(ref, "negative_features.csv")
    if not (pf and nf):
        parser.error("give -data DIR or both -pf FILE and -nf FILE")
    if not (args.gamma or args.gamma_scale):
        parser.error("give --gamma and / or --gamma_scale")
    positive = fileIO.read_feature_file(pf, normalize=True)[1]
    negative = fileIO.read_feature_file(nf, normalize=True)[1]
    scale = _lib.svm_gamma(np.vstack((positive, negative)), 'scale')
    gammas = list(args.gamma) + [m * scale for m in args.gamma_scale]
    table = grid(positive, negative, args.nu, gammas, folds=args.N_fold, seed=args.seed)
    save_grid(args.output_file or "svm_grid.csv", table, args=args)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
