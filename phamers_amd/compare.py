"""
compare.py -- is a difference between two cells of a parameter grid real?  The grids (``combo_grid``, ``svm_grid``,
``bandwidth``, ``dbscan_grid``) end in tables of held-out ROC areas; their cells are scored on the SAME rows, so they are
strongly correlated and per-cell error bars do not answer the question.  This module gives the paired answer two ways:
DeLong's covariance of the areas (DeLong, DeLong & Clarke-Pearson 1988) and a stratified bootstrap that resamples the rows
once for all cells.  The reference has no such tool (its cross_validate_all_algorithms prints one AUC per method).

Definitions.  ``scores`` is (C, n) float64, one row per cell, columns in ``vstack(positive,
negative)`` order: the first ``n_pos`` = P columns are the positives x, the other N = n - P the negatives y.  Scores must be
finite; -0.0 == +0.0, as in the sort.

    twice-placements   t_pos[c][i] = 2 #{j : y_j < x_i} + #{j : y_j == x_i},  t_neg[c][j] = 2 #{i : x_i > y_j} +
                       #{i : x_i == y_j} (uint32); both sum to area2[c] = 2 P N AUC, what ``learning.roc_points`` returns
    Gram matrices      G10[a][b] = sum_i t_pos[a][i] t_pos[b][i],  G01[a][b] = sum_j t_neg[a][j] t_neg[b][j] (exact integers)
    covariance         num10 = P G10[a][b] - area2[a] area2[b],  num01 = N G01[a][b] - area2[a] area2[b],
                       cov[a][b] = (num10 (N - 1) + num01 (P - 1)) / (4 P^2 N^2 (P - 1) (N - 1)): Python integers, rounded
                       ONCE by float(Fraction(...)).  This is DeLong's S10 / P + S01 / N.  P >= 2 and N >= 2.
    a pair             delta(a, b) = (area2[a] - area2[b]) / (2 P N) and delta_variance(a, b) = cov[a][a] + cov[b][b] -
                       2 cov[a][b], each evaluated in rationals and rounded once (neighbouring cells cancel heavily; two
                       identical cells give exactly 0.0); z = delta / sqrt(delta_variance), p = erfc(|z| / sqrt(2));
                       delta_variance == 0 gives z = p = nan
    bootstrap          resample b draws P positives and N negatives with replacement: key(b, s) = splitmix64(splitmix64(seed)
                       ^ (2 b + s)), s = 0 positives, 1 negatives; draw t = 0 .. n_s - 1 picks the class's row
                       (splitmix64(key + t) * n_s) >> 64; w[row] = times drawn; area2_boot[b][c] = sum_ij w_i w_j
                       (2 [x_i > y_j] + [x_i == y_j]).  Every cell sees the same resample: that pairing is the point.
    intervals          auc_boot = area2_boot / (2 P N); percentile intervals are np.quantile(samples, [(1 - level) / 2,
                       (1 + level) / 2]); a pair's samples are (area2_boot[:, a] - area2_boot[:, b]) / (2 P N)

    delong(scores, n_pos)                          -> DeLong
    bootstrap(scores, n_pos, resamples, seed)      -> Bootstrap
    cells(scores, n_pos, baseline, ...)            -> the table: every cell against ``baseline``, both ways, one upload
    Comparison(scores, n_pos)                      -> the resident handle behind them (``delong()``, ``bootstrap()``, ``close()``)
    combo_cells / svm_cells / density_cells        -> the (C, n) matrix from what the sweeps return
    python -m phamers_amd.compare -data DIR | -pf FILE -nf FILE --k_neighbors V [V ...] --k_clusters V [V ...] -N FOLDS
                                    [--seed S] [--baseline KN KC] [--resamples B] [--level L] [--both_strands] [-out FILE]
                                    -> a CSV: k_neighbors, k_clusters and the table's columns

The p-values are raw: no correction for the number of cells compared.  Plots are out of scope.
"""
import argparse
import math
import os
from fractions import Fraction
from statistics import NormalDist

import numpy as np

from . import _lib, fileIO

COLUMNS = ("auc", "se", "ci_low", "ci_high", "delta", "delta_se", "z", "p", "boot_low", "boot_high", "boot_delta_low",
           "boot_delta_high")
MAX_CELLS = _lib.COMPARE_MAX_CELLS
BOOT_MAX_ROWS = _lib.COMPARE_BOOT_MAX_ROWS


def _check_scores(scores, n_pos, two_each=False, boot=False):
    """The (C, n) float64 matrix and P, or the ValueError the module raises before any device work."""
    s = np.ascontiguousarray(scores, dtype=np.float64)
    if s.ndim != 2:
        raise ValueError("scores must be (cells, rows), got shape %r" % (s.shape,))
    C, n = s.shape
    P = int(n_pos)
    if P != n_pos or not 1 <= P < n:
        raise ValueError("n_pos=%r does not split %d rows into two classes" % (n_pos, n))
    if not 1 <= C <= MAX_CELLS:
        raise ValueError("need 1 <= cells <= %d, got %d" % (MAX_CELLS, C))
    if two_each and (P < 2 or n - P < 2):
        raise ValueError("DeLong's covariance needs two rows of each class, got %d positive and %d negative" % (P, n - P))
    if boot and n > BOOT_MAX_ROWS:
        raise ValueError("the bootstrap holds at most %d rows, got %d" % (BOOT_MAX_ROWS, n))
    if not np.isfinite(s).all():
        raise ValueError("Input contains NaN or infinity.")
    return s, P


def _level(level):
    if not 0.0 < float(level) < 1.0:
        raise ValueError("level must lie in (0, 1), got %r" % (level,))
    return float(level)


class DeLong(object):
    """What ``delong`` returns: ``auc`` (C,), ``area2`` (list of Python ints), ``placements_positive`` (C, P) and
    ``placements_negative`` (C, N) uint32, ``gram_positive`` / ``gram_negative`` (C, C) uint64, ``covariance`` (C, C), ``se``
    (C,), and the methods below.  The covariance is kept as integers over one denominator; every float is one rounding."""

    def __init__(self, n_pos, n_neg, area2, t_pos, t_neg, g10, g01):
        P, N = int(n_pos), int(n_neg)
        self.n_pos, self.n_neg = P, N
        self.area2 = [int(a) for a in area2]
        self.placements_positive, self.placements_negative = t_pos, t_neg
        self.gram_positive, self.gram_negative = g10, g01
        C = len(self.area2)
        self._den = 4 * P * P * N * N * (P - 1) * (N - 1)
        self._num = [[0] * C for _ in range(C)]
        for a in range(C):
            for b in range(a, C):
                aa = self.area2[a] * self.area2[b]
                num = (P * int(g10[a][b]) - aa) * (N - 1) + (N * int(g01[a][b]) - aa) * (P - 1)
                self._num[a][b] = self._num[b][a] = num
        self.auc = np.array([float(Fraction(a, 2 * P * N)) for a in self.area2], dtype=np.float64)
        self.covariance = np.array([[float(Fraction(v, self._den)) for v in row] for row in self._num], dtype=np.float64)
        self.se = np.sqrt(np.diag(self.covariance))

    def interval(self, level=0.95):
        """(low, high) arrays: auc -+ NormalDist().inv_cdf((1 + level) / 2) se, not clipped to [0, 1]."""
        q = NormalDist().inv_cdf((1.0 + _level(level)) / 2.0)
        return self.auc - q * self.se, self.auc + q * self.se

    def delta(self, a, b):
        return float(Fraction(self.area2[a] - self.area2[b], 2 * self.n_pos * self.n_neg))

    def delta_variance(self, a, b):
        return float(Fraction(self._num[a][a] + self._num[b][b] - 2 * self._num[a][b], self._den))

    def z(self, a, b):
        v = self.delta_variance(a, b)
        return self.delta(a, b) / math.sqrt(v) if v > 0.0 else float('nan')

    def p_value(self, a, b):
        z = self.z(a, b)
        return math.erfc(abs(z) / math.sqrt(2.0)) if z == z else float('nan')

    def against(self, baseline):
        """Every cell minus cell ``baseline``: {delta, delta_variance, delta_se, z, p}, arrays of C."""
        C = len(self.area2)
        out = {"delta": np.array([self.delta(c, baseline) for c in range(C)]),
               "delta_variance": np.array([self.delta_variance(c, baseline) for c in range(C)]),
               "z": np.array([self.z(c, baseline) for c in range(C)]),
               "p": np.array([self.p_value(c, baseline) for c in range(C)])}
        out["delta_se"] = np.sqrt(out["delta_variance"])
        return out


class Bootstrap(object):
    """What ``bootstrap`` returns: ``area2`` (B, C) uint64, ``auc`` (B, C) = area2 / (2 P N), and the percentile intervals."""

    def __init__(self, n_pos, n_neg, area2):
        self.n_pos, self.n_neg, self.area2 = int(n_pos), int(n_neg), area2
        self.auc = area2.astype(np.float64) / float(2 * self.n_pos * self.n_neg)   # (area2 <= 2 P N < 2^53: one rounding)

    def interval(self, level=0.95):
        """(low, high) arrays of C: np.quantile over the resamples."""
        level = _level(level)
        q = np.quantile(self.auc, [(1.0 - level) / 2.0, (1.0 + level) / 2.0], axis=0)
        return q[0], q[1]

    def delta_samples(self, a, b):
        d = self.area2[:, a].astype(np.int64) - self.area2[:, b].astype(np.int64)
        return d.astype(np.float64) / float(2 * self.n_pos * self.n_neg)

    def delta_interval(self, a, b, level=0.95):
        level = _level(level)
        q = np.quantile(self.delta_samples(a, b), [(1.0 - level) / 2.0, (1.0 + level) / 2.0])
        return float(q[0]), float(q[1])


class Comparison(object):
    """The cells on the device: uploaded and sorted once (``_lib.Compare``), for ``delong()`` and ``bootstrap()`` in any
    order and any number of times.  ``close()`` twice does nothing; also a context manager."""

    def __init__(self, scores, n_pos):
        s, P = _check_scores(scores, n_pos)
        self.n_pos, self.n_neg, self.cells = P, s.shape[1] - P, s.shape[0]
        self._h = _lib.Compare(_lib.get_context(), s, P)

    def delong(self):
        if self.n_pos < 2 or self.n_neg < 2:
            raise ValueError("DeLong's covariance needs two rows of each class, got %d positive and %d negative"
                             % (self.n_pos, self.n_neg))
        t_pos, t_neg = self._h.placements()
        area2, g10, g01 = self._h.grams()
        return DeLong(self.n_pos, self.n_neg, area2, t_pos, t_neg, g10, g01)

    def bootstrap(self, resamples=2000, seed=0, _per_launch=0):
        if int(resamples) < 1:
            raise ValueError("resamples must be >= 1, got %r" % (resamples,))
        if self.n_pos + self.n_neg > BOOT_MAX_ROWS:
            raise ValueError("the bootstrap holds at most %d rows, got %d" % (BOOT_MAX_ROWS, self.n_pos + self.n_neg))
        return Bootstrap(self.n_pos, self.n_neg, self._h.bootstrap(seed, int(resamples), per_launch=_per_launch))

    def close(self):
        self._h.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def delong(scores, n_pos):
    """DeLong's covariance of the C areas; see the module's definitions.  ValueError, before any device work, for scores
    that are not finite ("Input contains NaN or infinity."), a shape that is not (C, n) with 1 <= C <= 256, an ``n_pos``
    that leaves a class with fewer than two rows."""
    s, P = _check_scores(scores, n_pos, two_each=True)
    with Comparison(s, P) as c:
        return c.delong()


def bootstrap(scores, n_pos, resamples=2000, seed=0, _per_launch=0):
    """The stratified bootstrap of the C areas over shared resamples; see the module's definitions.  ``_per_launch`` is for
    the tests (resamples per kernel launch): no result depends on it."""
    s, P = _check_scores(scores, n_pos, boot=True)
    if int(resamples) < 1:
        raise ValueError("resamples must be >= 1, got %r" % (resamples,))
    with Comparison(s, P) as c:
        return c.bootstrap(resamples, seed, _per_launch)


def cells(scores, n_pos, baseline=0, resamples=2000, seed=0, level=0.95):
    """Every cell against cell ``baseline``, from one upload and one set of sorts: a dict of arrays of C -- ``auc``, ``se``,
    ``ci_low`` / ``ci_high`` (DeLong's interval of the area), ``delta`` = auc - auc[baseline], ``delta_se``, ``z``, ``p``
    (DeLong's test of delta = 0, raw), ``boot_low`` / ``boot_high`` (percentile interval of the area) and
    ``boot_delta_low`` / ``boot_delta_high`` (of delta) -- beside ``baseline``.  The baseline's own row has delta 0, z and p nan."""
    s, P = _check_scores(scores, n_pos, two_each=True, boot=True)
    level = _level(level)
    if not 0 <= int(baseline) < s.shape[0]:
        raise ValueError("baseline=%r is not one of the %d cells" % (baseline, s.shape[0]))
    baseline = int(baseline)
    with Comparison(s, P) as c:
        d, b = c.delong(), c.bootstrap(resamples, seed)
    lo, hi = d.interval(level)
    pair = d.against(baseline)
    blo, bhi = b.interval(level)
    bd = np.array([b.delta_interval(k, baseline, level) for k in range(s.shape[0])])
    return {"auc": d.auc, "se": d.se, "ci_low": lo, "ci_high": hi, "delta": pair["delta"], "delta_se": pair["delta_se"],
            "z": pair["z"], "p": pair["p"], "boot_low": blo, "boot_high": bhi, "boot_delta_low": bd[:, 0],
            "boot_delta_high": bd[:, 1], "baseline": baseline}


# ---- the (C, n) matrix from what the sweeps return --------------------------------------------------------------------------
def combo_cells(sweep):
    """(Kn Kc, n) from a ``combo_grid.sweep``: the combo scores of every cell, k_neighbors outermost, as ``combo_grid.grid``
    orders them.  ``n_pos`` is the number of positive rows the sweep was given."""
    return np.array([sweep.combo_scores(i, j) for i in range(len(sweep.k_neighbors)) for j in range(len(sweep.k_clusters))],
                    dtype=np.float64)


def svm_cells(sweep, y):
    """(scores (Gm V, n), n_pos) from a ``svm.nusvc_sweep(X, y, ..., folds=N)``: the held-out decisions of every cell, gamma
    outermost as ``svm_grid.grid`` orders them, the rows of class ``classes_[1]`` moved to the front (in their order).  A
    cell with a status holds NaN: drop such rows of the matrix before comparing."""
    held = np.asarray(sweep.held_decision, dtype=np.float64)
    pos = np.asarray(y) == sweep.classes_[1]
    order = np.concatenate((np.flatnonzero(pos), np.flatnonzero(~pos)))
    return held.reshape(-1, held.shape[-1])[:, order], int(pos.sum())


def density_cells(log_densities):
    """(B+ B-, n) from ``bandwidth.held_out_log_densities``: cell (a, b) is L+(h+_a) - L-(h-_b), the density method's score,
    h+ outermost as ``bandwidth.grid`` orders them.  ``n_pos`` is the number of positive rows."""
    L = log_densities
    up = np.hstack((L["pos_under_pos"], L["neg_under_pos"]))
    un = np.hstack((L["pos_under_neg"], L["neg_under_neg"]))
    return np.array([up[a] - un[b] for a in range(len(up)) for b in range(len(un))], dtype=np.float64)


def mixture_cells(result):
    """(scores (Ks, n), n_pos) from a ``mixture.cross_validate``: the held-out scores l_+ - l_- of every K, positives first."""
    return np.asarray(result.scores, dtype=np.float64), int(result.n_pos)


# ---- the command line ---------------------------------------------------------------------------------------------------
def save_cells(filename, k_neighbors, k_clusters, table, args=None):
    """One 'k_neighbors,k_clusters,<COLUMNS>' row per cell (the two k as integers, the floats as ``repr`` prints them)
    under a '# ' comment header."""
    header = "paired ROC-area comparison against cell %d: " % table["baseline"] + ",".join(("k_neighbors", "k_clusters") + COLUMNS)
    if args is not None:
        header = fileIO.generate_summary(args, header=header).rstrip('\n')
    with open(filename, 'w') as f:
        f.write('# ' + header.replace('\n', '\n# ') + '\n')
        for i in range(len(table["auc"])):
            f.write('%d,%d,' % (int(k_neighbors[i]), int(k_clusters[i])) + ','.join(repr(float(table[c][i])) for c in COLUMNS) + '\n')


def _parser():
    parser = argparse.ArgumentParser(prog="python -m phamers_amd.compare", description=__doc__.split('\n\n')[0])
    parser.add_argument('-data', '--data_directory', help="Directory containing reference_features/")
    parser.add_argument('-pf', '--positive_features_file', help="Positive features file")
    parser.add_argument('-nf', '--negative_features_file', help="Negative features file")
    parser.add_argument('-out', '--output_file', help="Filename for the output CSV")
    parser.add_argument('--k_neighbors', nargs='+', type=int, required=True, help="the k_neighbors values of the grid")
    parser.add_argument('--k_clusters', nargs='+', type=int, required=True, help="the k_clusters values of the grid")
    parser.add_argument('-N', '--N_fold', type=int, required=True, help="Folds of the validator's split")
    parser.add_argument('--seed', type=int, default=None, help="Seed of the fold assignment and of the bootstrap (0 if not given)")
    parser.add_argument('--baseline', nargs=2, type=int, metavar=('KN', 'KC'), default=None,
                        help="the cell every other is compared with (default: 3 86 when in the grid, else the first cell)")
    parser.add_argument('--resamples', type=int, default=2000, help="bootstrap resamples")
    parser.add_argument('--level', type=float, default=0.95, help="coverage of the intervals")
    parser.add_argument('--both_strands', action='store_true',
                        help="Fold both feature files with their reverse complement before normalising")
    return parser


def main(argv=None):
    from . import combo_grid, kmer
    parser = _parser()
    args = parser.parse_args(argv)
    pf, nf = args.positive_features_file, args.negative_features_file
    if args.data_directory:
        ref = os.path.join(args.data_directory, "reference_features")
        pf, nf = pf or os.path.join(ref, "positive_features.csv"), nf or os.path.join(ref, "negative_features.csv")
    if not (pf and nf):
        parser.error("give -data DIR or both -pf FILE and -nf FILE")
    kn = np.repeat(args.k_neighbors, len(args.k_clusters)).tolist()
    kc = np.tile(args.k_clusters, len(args.k_neighbors)).tolist()
    pairs = list(zip(kn, kc))
    want = tuple(args.baseline) if args.baseline else (3, 86)
    if args.baseline and want not in pairs:
        parser.error("--baseline %d %d is not a cell of the grid" % want)
    baseline = pairs.index(want) if want in pairs else 0
    positive, negative = fileIO.read_feature_file(pf)[1], fileIO.read_feature_file(nf)[1]
    if args.both_strands:
        from . import transform_kmers
        positive, negative = transform_kmers.fold_strands(positive), transform_kmers.fold_strands(negative)
    positive, negative = kmer.normalize_counts(positive), kmer.normalize_counts(negative)
    sweep = combo_grid.sweep(positive, negative, args.k_neighbors, args.k_clusters, folds=args.N_fold, seed=args.seed)
    table = cells(combo_cells(sweep), len(positive), baseline=baseline, resamples=args.resamples,
                  seed=args.seed if args.seed is not None else 0, level=args.level)
    save_cells(args.output_file or "compare.csv", kn, kc, table, args=args)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
