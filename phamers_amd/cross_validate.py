"""
cross_validate.py -- N-fold cross validation of the reference matrices (the other caller of the scoring path,
PhaMers' scripts/cross_validate.py:38-101) as a batched service on ONE resident GPU model.

The reference rebuilds everything per fold: it slices the train rows out of the matrices, refits k-means, fits a
k-NN classifier and scores the held-out rows -- N times, although the N train sets share (N-1)/N of their rows.
Here the full reference matrix is uploaded and prepared ONCE (`_lib.Model` over every positive and negative row); a
fold is then
    * a column mask over that model's train rows (the held-out rows are excluded from the k-NN search and, for the
      density method, from both kernel density sums and their row counts),
    * the fold's centroids, written into the model's centroid segments (k-means on the fold's train rows: scikit-learn
      by default, as the reference; ``kmeans='gpu'`` selects the deterministic device k-means per fold; kmeans and
      combo only),
    * for the svm method, a NuSVC fit on the rows the mask leaves in (phk_model_fit_svm),
    * one scoring call for the held-out rows.
The dbscan method runs through the reference's per-fold calls of phamer.score_points.  The likelihood method (this
project's own; ``positive_counts`` / ``negative_counts``, the integer rows) is one call of likelihood.cross_validate: the
fold is a group id on the queries and on the table's rows.
Scores are those of a model built from the fold's train rows alone (the k-NN search is translation invariant: only
the error bounds depend on the centring vector, and they are evaluated for the one in use);
tests/golden/cross_validation.npz holds what the reference's own cross_validate produced.

    validator = cross_validator(); validator.positive_data = ...; validator.negative_data = ...
    positive_scores, negative_scores = validator.cross_validate()

The reference shuffles the fold assignment with the unseeded global NumPy generator (scripts/cross_validate.py:71-78);
``seed`` makes a run reproducible with the same draws (np.random.seed(seed) right before its two shuffles).  A custom
``scoring_function`` (anything but phamer.score_points) is honoured with the reference's per-fold calls.
"""
import logging
import os

import numpy as np

from . import _lib
from . import learning
from . import phamer

logger = logging.getLogger(__name__)
logger.setLevel(logging.WARNING)


ALL_METHODS = ('dbscan', 'kmeans', 'knn', 'svm', 'density', 'combo')   # scripts/cross_validate.py:304


class FoldPlan(object):
    """Which fold every positive / negative row is held out in."""

    def __init__(self, n_positive, n_negative, folds, seed=None):
        self.folds = int(folds)
        self.positive = np.arange(n_positive) % self.folds
        self.negative = np.arange(n_negative) % self.folds
        rng = np.random if seed is None else np.random.RandomState(seed)   # RandomState(seed) == np.random.seed(seed)
        rng.shuffle(self.positive)
        rng.shuffle(self.negative)

    def held_out(self, fold):
        return self.positive == fold, self.negative == fold


class cross_validator(object):

    def __init__(self):
        self.positive_data = self.negative_data = None
        self.positive_counts = self.negative_counts = None   # the integer count rows: what method 'likelihood' scores
        self.positive_ids = self.negative_ids = None
        self.positive_scores = self.negative_scores = None
        self.equalize_reference = False
        self.N = 20                                  # scripts/cross_validate.py:48
        self.method = 'combo'
        self.scoring_function = phamer.score_points  # scripts/cross_validate.py:275
        self.seed = None
        self.kmeans = 'sklearn'                      # or 'gpu': deterministic device k-means per fold
        self.k_clusters = 86                         # scripts/phamer.py:78
        self.k_neighbors = 3                         # scripts/phamer.py:79
        self.positive_bandwidth = 0.005              # scripts/phamer.py:82-83 (method 'density')
        self.negative_bandwidth = 0.01
        self.svm_nu = 0.5                            # NuSVC()'s defaults (method 'svm'); svm_grid.py tables other values
        self.svm_gamma = 'scale'
        self.pseudocount = 0.5                       # method 'likelihood' (likelihood.py)
        self.likelihood_per_kmer = False
        self.score_threshold = 0                    # scripts/cross_validate.py:53
        self.output_directory = "cross_validation"   # scripts/cross_validate.py:55
        self.methods = list(ALL_METHODS)             # what cross_validate_all_algorithms runs (scripts/cross_validate.py:304)

    # ---- the reference's entry point ----------------------------------------------------------------------
    def cross_validate(self):
        """Every reference row scored by a model that has not seen its fold (scripts/cross_validate.py:57-101).
        Returns (positive_scores, negative_scores)."""
        self._equalize()
        if self.method == 'likelihood' and self.scoring_function is phamer.score_points:
            return self._likelihood_folds()
        self.num_positive, self.num_negative = self.positive_data.shape[0], self.negative_data.shape[0]
        plan = FoldPlan(self.num_positive, self.num_negative, self.N, self.seed)
        self.positive_assignment, self.negative_assignment = plan.positive, plan.negative
        resident = self.scoring_function is phamer.score_points and (self.method or 'combo') in ('knn', 'kmeans', 'combo', 'density', 'svm')
        runner = self._folds_on_resident_model if resident else self._folds_through_scoring_function
        self.positive_scores, self.negative_scores = runner(plan)
        logger.info("%d-fold cross validation complete." % self.N)
        return self.positive_scores, self.negative_scores

    def _equalize(self):
        """First min(n+, n-) rows of each class when asked to (scripts/cross_validate.py:63-69)."""
        if not self.equalize_reference:
            return
        m = min(self.positive_data.shape[0], self.negative_data.shape[0])
        self.positive_data, self.negative_data = self.positive_data[:m], self.negative_data[:m]
        self.positive_ids = None if self.positive_ids is None else self.positive_ids[:m]
        self.negative_ids = None if self.negative_ids is None else self.negative_ids[:m]
        if self.positive_counts is not None and self.negative_counts is not None:
            self.positive_counts, self.negative_counts = self.positive_counts[:m], self.negative_counts[:m]

    def _likelihood_folds(self):
        """Method 'likelihood': the count rows, every fold excluded by its group id in ONE device call
        (likelihood.cross_validate on this run's FoldPlan)."""
        from . import likelihood
        if self.positive_counts is None or self.negative_counts is None:
            raise ValueError("method 'likelihood' needs the integer count rows (positive_counts / negative_counts): "
                             "positive_data / negative_data hold frequencies only")
        self.num_positive, self.num_negative = len(self.positive_counts), len(self.negative_counts)
        plan = FoldPlan(self.num_positive, self.num_negative, self.N, self.seed)
        self.positive_assignment, self.negative_assignment = plan.positive, plan.negative
        self.positive_scores, self.negative_scores = likelihood.cross_validate(
            self.positive_counts, self.negative_counts, self.N, self.seed, self.pseudocount, self.likelihood_per_kmer,
            _plan=plan)
        logger.info("%d-fold cross validation complete." % self.N)
        return self.positive_scores, self.negative_scores

    # ---- batched: one model, a fold = mask + centroids ---------------------------------------------------------
    def _fold_centroids(self, train_rows):
        if self.kmeans == 'gpu':
            return learning.kmeans_gpu(train_rows, self.k_clusters)[1]
        return learning.get_centroids(train_rows, learning.kmeans(train_rows, self.k_clusters))

    def _folds_on_resident_model(self, plan):
        method = self.method or 'combo'
        P = np.ascontiguousarray(self.positive_data, dtype=np.float64)
        Nm = np.ascontiguousarray(self.negative_data, dtype=np.float64)
        if np.isnan(P).any() or np.isnan(Nm).any():
            raise ValueError("Input contains NaN.")
        pos_scores, neg_scores = np.zeros(len(P)), np.zeros(len(Nm))
        with_centroids = method in ('kmeans', 'combo')
        model = None
        ctx = _lib.get_context()
        self.model_uploads = 0
        try:
            for fold in range(plan.folds):
                logger.info('Iteration %d/%d' % (1 + fold, plan.folds))
                out_p, out_n = plan.held_out(fold)
                cents = None
                if with_centroids:
                    cents = self._fold_centroids(P[~out_p]), self._fold_centroids(Nm[~out_n])
                if model is not None and with_centroids and (
                        len(cents[0]), len(cents[1])) != (self._model_centroids[0], self._model_centroids[1]):
                    model.close()      # a fit that came back with another number of clusters: rebuild (rare)
                    model = None
                if model is None:
                    model = _lib.Model(ctx, P, Nm, cents[0] if cents else None, cents[1] if cents else None,
                                       k_neighbors=self.k_neighbors)
                    self._model_centroids = (len(cents[0]), len(cents[1])) if cents else (0, 0)
                    self.model_uploads += 1
                    if method == 'density':
                        model.set_bandwidths(self.positive_bandwidth, self.negative_bandwidth)
                elif with_centroids:
                    model.set_centroids(*cents)
                model.set_column_mask(np.concatenate((out_p, out_n)))
                if method == 'svm':
                    # on the fold's train rows (the mask's complement); 'scale' / 'auto' are taken over those rows
                    model.fit_svm(self.svm_nu, self.svm_gamma)
                scores = model.score(np.vstack((P[out_p], Nm[out_n])), method)
                n_p = int(out_p.sum())
                pos_scores[out_p], neg_scores[out_n] = scores[:n_p], scores[n_p:]
        finally:
            if model is not None:
                model.close()
        return pos_scores, neg_scores

    # ---- generic: any scoring function, the reference's per-fold calls ---------------------------------------
    def _folds_through_scoring_function(self, plan):
        # (phamer.score_points serves knn / kmeans / combo / density only; the reference's call of it for the other methods
        # is score_with_scorer -- the same scorer, the same matrices)
        fn = phamer.score_with_scorer if self.scoring_function is phamer.score_points else self.scoring_function
        pos_scores, neg_scores = np.zeros(self.num_positive), np.zeros(self.num_negative)
        for fold in range(plan.folds):
            out_p, out_n = plan.held_out(fold)
            scores = fn(np.vstack((self.positive_data[out_p], self.negative_data[out_n])),
                                           self.positive_data[~out_p], self.negative_data[~out_n], method=self.method)
            scores = np.asarray(scores)
            if scores.ndim == 2 and scores.shape[1] == 1:
                scores = scores[:, 0]    # the dbscan method's (n, 1) scores (the NumPy of the reference's era took them)
            n_p = int(out_p.sum())
            pos_scores[out_p], neg_scores[out_n] = scores[:n_p], scores[n_p:]
        return pos_scores, neg_scores

    # ---- evaluation of the last run (scripts/cross_validate.py:135-238; the plots stay out) ---------------
    def performance(self):
        """(fpr, tpr, auc) of the last run's scores: learning.predictor_performance, what the reference's plot_ROC draws."""
        if self.positive_scores is None or self.negative_scores is None:
            raise ValueError("performance: no scores yet, call cross_validate() first")
        return learning.predictor_performance(self.positive_scores, self.negative_scores)

    def _open_output(self, file_name):
        directory = os.path.dirname(file_name)
        if directory and not os.path.isdir(directory):
            os.makedirs(directory)
        return open(file_name, 'w')

    def make_metrics_file(self):
        """metrics.txt (scripts/cross_validate.py:156-172): the header line, then one ``name<TAB>value`` line per metric of
        learning.get_predictor_metrics at ``score_threshold``, values by ``repr``.  (The reference appends a pandas
        Series.to_csv to the header: the same lines under a pandas-version dependent column line, which is not written.)"""
        metrics = learning.get_predictor_metrics(self.positive_scores, self.negative_scores, threshold=self.score_threshold)
        with self._open_output(self.get_metric_filename()) as f:
            f.write("# Cross Validation Performance Metrics\n")
            for name in learning.METRIC_NAMES:
                f.write("%s\t%r\n" % (name, metrics[name]))

    def make_summary_file(self, id_label_map=None):
        """scores.txt (scripts/cross_validate.py:174-192): every positive id with its score, ascending, and its label when a
        map is given -- the reference's text.  The order is the device argsort of the scores (learning.argsort_scores,
        stable): ids with equal scores stay in ``positive_ids`` order, which is what the reference's
        ``sorted(zip(score, id))`` gives when the ids of tied scores already ascend as strings; where they do not, the
        reference orders the tied ids as strings and this file keeps them in input order."""
        scores = np.asarray(self.positive_scores, dtype=np.float64)
        order = learning.argsort_scores(scores)
        text = "# Cross Validation Scores"
        for i in order:
            id, score = self.positive_ids[i], scores[i]
            if id_label_map is None:
                text += "\n{id}\t{score}".format(id=id, score=score)
            else:
                text += "\n{id}\t{score}\t{label}".format(id=id, score=score, label=id_label_map[id])
        with self._open_output(self.get_summary_filename()) as f:
            f.write(text)

    def cross_validate_all_algorithms(self):
        """{method: (fpr, tpr, auc)} for every method of ``self.methods`` (scripts/cross_validate.py:194-222 without the
        plot).  Each method runs ``cross_validate()`` afresh: with ``seed`` set all of them use the same fold plan."""
        results = {}
        for method in self.methods:
            self.method = method
            logger.info("%d-Fold Cross Validation" % self.N)
            logger.info("Algorithm: %s" % method.upper())
            positive_scores, negative_scores = self.cross_validate()
            results[method] = learning.predictor_performance(positive_scores, negative_scores)
        return results

    # filename makers (scripts/cross_validate.py:224-238)
    def get_metric_filename(self):
        return os.path.join(self.output_directory, "metrics.txt")

    def get_summary_filename(self):
        return os.path.join(self.output_directory, "scores.txt")

    def get_all_algorithms_filename(self):
        return os.path.join(self.output_directory, "all_algorithms_auc.txt")


def _parser():
    import argparse
    parser = argparse.ArgumentParser(description="This script is for doing N-fold cross validation of the Phamer scoring algorithm",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    input_group = parser.add_argument_group("Inputs")
    input_group.add_argument('-pf', '--positive_features_file', required=True, help="Positive features file")
    input_group.add_argument('-nf', '--negative_features_file', required=True, help="Negative features file")
    output_group = parser.add_argument_group("Outputs")
    output_group.add_argument('-out', '--output_directory', default="cross_validation", help="Output directory")
    options_group = parser.add_argument_group("Options")
    options_group.add_argument('-N', '--N_fold', default=20, type=int, help="Number of iteration in N-fold cross validation")
    options_group.add_argument('-m', '--method', default='combo', help="Scoring algorithm method")
    options_group.add_argument('-a', '--test_all', action='store_true', help="Flag to cross validate all algorithms")
    options_group.add_argument('-l', '--labels_file', help="Label file mapping id to label")
    options_group.add_argument('-equal', '--equalize_reference', action='store_true', help="Use same number of reference data from each")
    options_group.add_argument('--seed', type=int, default=None, help="Seed of the fold assignment (unseeded as the reference when absent)")
    options_group.add_argument('--kmeans', default='sklearn', choices=('sklearn', 'gpu'), help="Per-fold k-means fit")
    options_group.add_argument('--both_strands', action='store_true',
                               help="Fold both feature files with their reverse complement before normalising")
    # (long options only, as in phamers_amd.phamer, where -k is the k-mer length; absent, the validator keeps its own values)
    options_group.add_argument('--k_neighbors', type=int, default=argparse.SUPPRESS, metavar='K',
                               help="Neighbours of the k-NN vote (the validator's default: 3; combo_grid.py tables others)")
    options_group.add_argument('--k_clusters', type=int, default=argparse.SUPPRESS, metavar='K',
                               help="Clusters per class of the per-fold k-means fit (the validator's default: 86)")
    console_options_group = parser.add_argument_group("Console Options")
    console_options_group.add_argument('-v', '--verbose', action='store_true', default=False, help="Verbose output")
    console_options_group.add_argument('--debug', action='store_true', default=False, help="Debug console")
    return parser


def main(argv=None):
    """The reference's command line (scripts/cross_validate.py:240-307) without its plots: metrics.txt and scores.txt in the
    output directory, with -a also all_algorithms_auc.txt (``method<TAB>repr(auc)`` per line).  --seed and --kmeans are
    this project's additions, and so are --both_strands and --k_neighbors / --k_clusters (4.18)."""
    from . import fileIO, kmer
    parser = _parser()
    args = parser.parse_args(argv)
    logger.setLevel(logging.DEBUG if args.debug else logging.INFO if args.verbose else logging.WARNING)

    validator = cross_validator()
    validator.method, validator.N = args.method, args.N_fold
    validator.output_directory = args.output_directory
    validator.seed, validator.kmeans = args.seed, args.kmeans
    phamer._apply_k_options(validator, args)
    validator.positive_ids, positive_data = fileIO.read_feature_file(args.positive_features_file)
    validator.negative_ids, negative_data = fileIO.read_feature_file(args.negative_features_file)
    if args.both_strands:
        from . import transform_kmers
        positive_data, negative_data = transform_kmers.fold_strands(positive_data), transform_kmers.fold_strands(negative_data)
    validator.positive_counts, validator.negative_counts = positive_data, negative_data
    validator.positive_data = kmer.normalize_counts(positive_data)
    validator.negative_data = kmer.normalize_counts(negative_data)
    validator.equalize_reference = args.equalize_reference
    validator.cross_validate()
    validator.make_metrics_file()
    id_label_map = fileIO.read_label_file(args.labels_file) if args.labels_file else None
    validator.make_summary_file(id_label_map=id_label_map)
    if args.test_all:
        validator.methods = list(ALL_METHODS)
        results = validator.cross_validate_all_algorithms()
        with validator._open_output(validator.get_all_algorithms_filename()) as f:
            for method in validator.methods:
                f.write("%s\t%r\n" % (method, results[method][2]))
    logger.info("Cross validation complete.")
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
