"""
combo_grid.py -- the table behind a choice of ``k_neighbors`` and ``k_clusters`` (``phamer_scorer``'s and
``cross_validator``'s attributes of those names) for the knn, kmeans and combo scoring methods: the held-out ROC area and
accuracy of every cell of a grid k_neighbors x k_clusters, what svm_grid.py is to the svm method's parameters, bandwidth.py
to the density method's and dbscan_grid.py to ``eps`` / ``min_samples``.

    sweep(positive, negative, k_neighbors, k_clusters, folds, seed=None)
                                    -> the held-out knn votes (one row per k_neighbors value), k-means metrics (one row per
                                       k_clusters value), their sums per cell, and every AUC / accuracy
    grid(...same arguments...)      -> one entry per cell, k_neighbors outermost: k_neighbors, k_clusters, knn_auc,
                                       kmeans_auc, auc, accuracy
    python -m phamers_amd.combo_grid -data DIR | -pf FILE -nf FILE --k_neighbors V [V ...] --k_clusters V [V ...]
                                    -N FOLDS [--seed S] [--both_strands] [-out FILE]
                                    -> a CSV of those columns

The reference fixes ``k_neighbors = 3`` and ``k_clusters = 86`` (scripts/phamer.py:78-79); its only study of k is the mean
silhouette (scripts/cluster.py, ``cluster.silhouette_curve``), which does not ask how well the scorer separates the classes.
A row is scored by the model of the fold that held it out, in the validator's own split (``cross_validate.FoldPlan``): a cell
equals ``cross_validator`` with that ``k_neighbors`` / ``k_clusters``, ``N = folds`` and the same ``seed`` (bit for bit on
the exact route).  The rows go up once; every fold's k-means of every k runs side by side on the
device (a fit the device declines goes through ``learning.kmeans`` on the host), the neighbour pass does not grow with the
number of ``k_neighbors`` values, and the centroid pass serves every ``k_clusters`` value at once.  Plots are out of scope
(DESIGN.md section 7): the table is written as a CSV.
"""
import argparse
import os
import time

import numpy as np

from . import _lib, cross_validate, fileIO, learning

COLUMNS = ("k_neighbors", "k_clusters", "knn_auc", "kmeans_auc", "auc", "accuracy")
POSITIVE, NEGATIVE = 1, 0   # the class of a key of ``centroids``


class ComboSweep(object):
    """What ``sweep`` returns (its docstring lists the fields)."""

    def combo_scores(self, i, j):
        """The combo method's scores at ``k_neighbors[i]``, ``k_clusters[j]`` (scripts/phamer.py:313)."""
        return self.knn_scores[i] + self.kmeans_scores[j]


def _int_list(values, name):
    a = np.asarray(values if values is not None else [])
    if a.size and not np.all(np.asarray(a, dtype=np.float64) == np.round(np.asarray(a, dtype=np.float64))):
        raise ValueError("%s must be integers, got %r" % (name, a.tolist()))
    return [int(v) for v in a.ravel().tolist()]


def _evaluate(scores, n_pos):
    """(auc, accuracy at threshold 0) of one score vector in vstack(positive, negative) order."""
    pos, neg = scores[:n_pos], scores[n_pos:]
    tp, fp, fn, tn = learning.truth_counts(pos, neg, threshold=0)   # (the counts behind learning.get_truth_table)
    return learning.predictor_performance(pos, neg)[2], float(tp + tn) / (tp + fp + fn + tn)


def sweep(positive, negative, k_neighbors, k_clusters, folds, seed=None, _chunk=0, _rows_per_pass=0, _details=None):
    """Every row of ``positive`` / ``negative`` scored by the model of the fold that holds it out in
    ``cross_validate.FoldPlan(n_pos, n_neg, folds, seed)``, for every value of ``k_neighbors`` (Kn values) and ``k_clusters``
    (Kc values), in one call.  Returns an object with

      ``k_neighbors``, ``k_clusters``    the values as given (duplicates and order kept), ``plan`` the FoldPlan
      ``knn_scores`` (Kn, n_pos + n_neg) the knn method's votes, +-1.0, rows in ``vstack(positive, negative)`` order
      ``kmeans_scores`` (Kc, n_pos + n_neg) the kmeans method's scores; ``combo_scores(i, j)`` = their sum
      ``knn_auc``, ``knn_accuracy`` (Kn,); ``kmeans_auc``, ``kmeans_accuracy`` (Kc,); ``combo_auc``, ``combo_accuracy``
      (Kn, Kc): ``learning.predictor_performance``'s area, and (tp + tn) / rows of the truth table at threshold 0
      ``centroids[(fold, cls, j)]``      the fold's centroids of class ``cls`` (POSITIVE = 1, NEGATIVE = 0) at k_clusters[j]
      ``problems``, ``routes``           the k-means problems as (fold, cls, k) and, for each, 'device' or 'host' (the device
                                         declined as in ``learning.kmeans_sweep``: the fit went through ``learning.kmeans``)

    Either list may be empty: that half is skipped (its fields are empty).  ValueError, before any device work, when both
    are, for non-finite rows ("Input contains NaN."), ``folds < 2``, a ``k_neighbors`` outside 1..min(64, smallest train set
    of a fold), a ``k_clusters`` outside 1..(smallest train set of one class).  PHAMERS_KMEANS=sklearn sends every k-means
    problem through the host route; PHAMERS_KMEANS=gpu (other seeds than the reference's) is not supported here.  The ``_``
    arguments are for the tests: k-means problems per launch, query rows per launch of the pair passes."""
    mode = os.environ.get("PHAMERS_KMEANS", "device")
    if mode == "gpu":
        raise NotImplementedError("combo_grid.sweep reproduces the reference's seeds; PHAMERS_KMEANS=gpu selects others")
    P = np.ascontiguousarray(positive, dtype=np.float64)
    Nm = np.ascontiguousarray(negative, dtype=np.float64)
    if P.ndim != 2 or Nm.ndim != 2 or P.shape[1] != Nm.shape[1] or P.shape[1] < 1:
        raise ValueError("positive and negative rows must be 2-D with the same number of columns")
    if not (np.isfinite(P).all() and np.isfinite(Nm).all()):
        raise ValueError("Input contains NaN.")
    if folds is None or int(folds) < 2:
        raise ValueError("the grid needs folds >= 2, got %r" % (folds,))
    kn, kc = _int_list(k_neighbors, "k_neighbors"), _int_list(k_clusters, "k_clusters")
    if not kn and not kc:
        raise ValueError("give at least one k_neighbors or one k_clusters value")
    n_pos, n_neg, D, F = len(P), len(Nm), P.shape[1], int(folds)
    M = n_pos + n_neg
    if M > _lib.COMBO_GRID_MAX_ROWS:
        raise ValueError("at most %d rows, got %d" % (_lib.COMBO_GRID_MAX_ROWS, M))
    plan = cross_validate.FoldPlan(n_pos, n_neg, F, seed)
    held_p, held_n = np.bincount(plan.positive, minlength=F), np.bincount(plan.negative, minlength=F)
    train = (n_pos - held_p, n_neg - held_n)           # train-set sizes per slot (0: positive) and fold
    kn_max = min(_lib.COMBO_GRID_MAX_NEIGHBORS, int((train[0] + train[1]).min()))
    for k in kn:
        if not 1 <= k <= kn_max:
            raise ValueError("k_neighbors=%d out of range (1..min(%d, smallest train set = %d))"
                             % (k, _lib.COMBO_GRID_MAX_NEIGHBORS, int((train[0] + train[1]).min())))
    kc_max = int(min(train[0].min(), train[1].min()))
    for k in kc:
        if not 1 <= k <= kc_max:
            raise ValueError("k_clusters=%d out of range (1..smallest train set of a class = %d)" % (k, kc_max))

    X = np.vstack((P, Nm))
    fold_of = np.concatenate((plan.positive, plan.negative)).astype(np.uint32)
    is_pos = np.r_[np.ones(n_pos, dtype=np.uint8), np.zeros(n_neg, dtype=np.uint8)]
    ku = list(dict.fromkeys(kc))                       # the distinct values, first seen first: one bank segment each
    koff = np.concatenate(([0], np.cumsum(ku))).astype(np.int64)
    Ksum = int(koff[-1])
    Cb = 2 * Ksum

    def train_rows(slot, fold):
        return np.flatnonzero((is_pos == (1 - slot)) & (fold_of != fold))

    out = ComboSweep()
    out.k_neighbors, out.k_clusters, out.plan = kn, kc, plan
    out.problems, out.routes, out.centroids = [], [], {}
    clock = {"fit": 0.0, "host_routes": 0.0, "score": 0.0}   # seconds per stage, for tools/bench_combo_grid.py
    t_start = time.perf_counter()
    ctx = _lib.get_context()
    cg = _lib.ComboGrid(ctx, X, fold_of, is_pos, F)
    try:
        if ku:
            # per train set: NumPy's column mean and the stopping tolerance, as learning.kmeans_reference_on_device forms them
            set_mean, set_tol = np.zeros((2 * F, D)), np.zeros(2 * F)
            for slot in range(2):
                for f in range(F):
                    T = X[train_rows(slot, f)]
                    set_mean[slot * F + f] = T.mean(axis=0)
                    T -= set_mean[slot * F + f]
                    set_tol[slot * F + f] = float(np.mean(np.var(T, axis=0)) * 1e-4)
            problems = [(slot, f, j) for slot in range(2) for f in range(F) for j in range(len(ku))]
            bank_off = [f * Cb + slot * Ksum + int(koff[j]) for slot, f, j in problems]
            on_device = [i for i, (slot, f, j) in enumerate(problems)
                         if mode != "sklearn" and ku[j] < learning.SWEEP_MAX_K and D >= 2]   # (one column: NumPy sums pairwise)
            drawn = {}
            for i in on_device:
                slot, f, j = problems[i]
                key = (int(train[slot][f]), ku[j])
                if key not in drawn:
                    drawn[key] = learning.placement_draws(*key)
            keys = [(int(train[problems[i][0]][problems[i][1]]), ku[problems[i][2]]) for i in on_device]
            t0 = time.perf_counter()
            fit = cg.fit([problems[i][0] * F + problems[i][1] for i in on_device], [k for _, k in keys],
                         [drawn[key][0] for key in keys], [drawn[key][1] for key in keys], set_mean, set_tol, F * Cb,
                         [bank_off[i] for i in on_device], chunk=_chunk)
            clock["fit"] = time.perf_counter() - t0
            if _details is not None:
                _details.update(fit)
                _details["on_device"] = [problems[i] for i in on_device]
            where = {i: n for n, i in enumerate(on_device)}
            host_centroids = {}
            t0 = time.perf_counter()
            for i, (slot, f, j) in enumerate(problems):
                n = where.get(i)
                host = n is None or bool(fit["status"][n]) or not (fit["seed_margin"][n] >= learning.SEED_MIN_MARGIN) \
                    or not (fit["min_gap"][n] >= learning.KMEANS_MIN_GAP)
                if host:
                    T = X[train_rows(slot, f)]
                    C = np.asarray(learning.get_centroids(T, learning.kmeans(T, ku[j])), dtype=np.float64)
                    host_centroids[i] = C
                    # (a host fit that came back with fewer clusters: the segment's spare rows repeat its first centroid,
                    # which leaves every minimum what it is)
                    cg.put_centroids(bank_off[i], np.vstack((C, np.repeat(C[:1], ku[j] - len(C), axis=0))))
                out.problems.append((f, 1 - slot, ku[j]))
                out.routes.append("host" if host else "device")
            clock["host_routes"] = time.perf_counter() - t0
            bank = cg.get_centroids(0, F * Cb)
            index = {(slot, f, j): i for i, (slot, f, j) in enumerate(problems)}
            for jj, k in enumerate(kc):
                j = ku.index(k)
                for slot in range(2):
                    for f in range(F):
                        i = index[(slot, f, j)]
                        out.centroids[(f, 1 - slot, jj)] = host_centroids[i] if i in host_centroids \
                            else bank[bank_off[i]:bank_off[i] + k].copy()
        t0 = time.perf_counter()
        knn, km = cg.score(kn, ku, rows_per_pass=_rows_per_pass)
        clock["score"] = time.perf_counter() - t0
    finally:
        cg.close()
    t0 = time.perf_counter()
    out.knn_scores = knn
    out.kmeans_scores = km[[ku.index(k) for k in kc]] if kc else np.empty((0, M))
    ev = [_evaluate(s, n_pos) for s in out.knn_scores]
    out.knn_auc, out.knn_accuracy = np.array([e[0] for e in ev]), np.array([e[1] for e in ev])
    ev = [_evaluate(s, n_pos) for s in out.kmeans_scores]
    out.kmeans_auc, out.kmeans_accuracy = np.array([e[0] for e in ev]), np.array([e[1] for e in ev])
    ev = [_evaluate(out.combo_scores(i, j), n_pos) for i in range(len(kn)) for j in range(len(kc))]
    out.combo_auc = np.array([e[0] for e in ev]).reshape(len(kn), len(kc))
    out.combo_accuracy = np.array([e[1] for e in ev]).reshape(len(kn), len(kc))
    clock["evaluate"] = time.perf_counter() - t0
    clock["total"] = time.perf_counter() - t_start
    if _details is not None:
        _details["seconds"] = clock
    return out


def grid(positive, negative, k_neighbors, k_clusters, folds, seed=None):
    """The table as a dict of arrays, one entry per cell in the order ``for kn in k_neighbors: for kc in k_clusters``:
    ``k_neighbors``, ``k_clusters``, ``knn_auc`` and ``kmeans_auc`` (the two halves alone at the cell's values), ``auc`` and
    ``accuracy`` of the combo method, and ``best``: the index of the cell of largest ``auc``, the first such cell on a tie.
    Both lists must have a value (``sweep`` serves one half alone)."""
    kn, kc = _int_list(k_neighbors, "k_neighbors"), _int_list(k_clusters, "k_clusters")
    if not kn or not kc:
        raise ValueError("the table needs at least one k_neighbors and one k_clusters value")
    res = sweep(positive, negative, kn, kc, folds, seed=seed)
    auc = res.combo_auc.ravel()
    return {"k_neighbors": np.repeat(np.array(kn, dtype=np.float64), len(kc)),
            "k_clusters": np.tile(np.array(kc, dtype=np.float64), len(kn)),
            "knn_auc": np.repeat(res.knn_auc, len(kc)), "kmeans_auc": np.tile(res.kmeans_auc, len(kn)),
            "auc": auc, "accuracy": res.combo_accuracy.ravel(), "best": int(np.argmax(auc))}


def save_grid(filename, table, args=None):
    """One 'k_neighbors,k_clusters,knn_auc,kmeans_auc,auc,accuracy' row per cell (the two k as integers, the floats as
    ``repr`` prints them) under a '# ' comment header."""
    header = "k_neighbors x k_clusters grid: " + ",".join(COLUMNS)
    if args is not None:
        header = fileIO.generate_summary(args, header=header).rstrip('\n')
    with open(filename, 'w') as f:
        f.write('# ' + header.replace('\n', '\n# ') + '\n')
        for i in range(len(table["auc"])):
            f.write('%d,%d,%r,%r,%r,%r\n' % (int(table["k_neighbors"][i]), int(table["k_clusters"][i]),
                                             float(table["knn_auc"][i]), float(table["kmeans_auc"][i]),
                                             float(table["auc"][i]), float(table["accuracy"][i])))


def read_grid(filename):
    """The per-cell arrays (and ``best``) of a file save_grid wrote."""
    rows = [line.strip().split(',') for line in open(filename) if not line.startswith('#') and line.strip()]
    out = {name: np.array([float(r[k]) for r in rows], dtype=np.float64) for k, name in enumerate(COLUMNS)}
    out["best"] = None if not rows or np.isnan(out["auc"]).all() else int(np.nanargmax(out["auc"]))
    return out


def _parser():
    parser = argparse.ArgumentParser(prog="python -m phamers_amd.combo_grid", description=__doc__.split('\n\n')[0])
    parser.add_argument('-data', '--data_directory', help="Directory containing reference_features/")
    parser.add_argument('-pf', '--positive_features_file', help="Positive features file")
    parser.add_argument('-nf', '--negative_features_file', help="Negative features file")
    parser.add_argument('-out', '--output_file', help="Filename for the output CSV")
    parser.add_argument('--k_neighbors', nargs='+', type=int, required=True, help="the k_neighbors values of the grid")
    parser.add_argument('--k_clusters', nargs='+', type=int, required=True, help="the k_clusters values of the grid")
    parser.add_argument('-N', '--N_fold', type=int, required=True, help="Folds of the validator's split")
    parser.add_argument('--seed', type=int, default=None, help="Seed of the fold assignment")
    parser.add_argument('--both_strands', action='store_true',
                        help="Fold both feature files with their reverse complement before normalising")
    return parser


def main(argv=None):
    from . import kmer
    parser = _parser()
    args = parser.parse_args(argv)
    pf, nf = args.positive_features_file, args.negative_features_file
    if args.data_directory:
        ref = os.path.join(args.data_directory, "reference_features")
        pf, nf = pf or os.path.join(ref, "positive_features.csv"), nf or os.path.join(ref, "negative_features.csv")
    if not (pf and nf):
        parser.error("give -data DIR or both -pf FILE and -nf FILE")
    positive, negative = fileIO.read_feature_file(pf)[1], fileIO.read_feature_file(nf)[1]
    if args.both_strands:
        from . import transform_kmers
        positive, negative = transform_kmers.fold_strands(positive), transform_kmers.fold_strands(negative)
    positive, negative = kmer.normalize_counts(positive), kmer.normalize_counts(negative)
    table = grid(positive, negative, args.k_neighbors, args.k_clusters, folds=args.N_fold, seed=args.seed)
    save_grid(args.output_file or "combo_grid.csv", table, args=args)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
