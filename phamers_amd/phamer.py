"""
phamer.py -- drop-in for the scoring entry points of PhaMers' scripts/phamer.py, device resident.

    phamer_scorer            attribute surface + load_data / screen_by_length / equalize_reference_data /
                             score_points / dbscan_ / knn_ / kmeans_ / svm_ / density_ / combo_score_points
                                                                                    scripts/phamer.py:42-313
    score_points(scoring_data, positive_training_data, negative_training_data, method=None)
                                                                                    scripts/phamer.py:451-468
    main()                   `python -m phamers_amd.phamer -in <dir> -data <dir> [-e]`  scripts/phamer.py:512-598

Data path.  A FASTA input is parsed once by the native reader, its bases are uploaded once, and from there the
contigs live on the GPU as a `_lib.Batch` (uint32 counts + row sums in HBM): the length screen is a device row
gather, scoring runs on the resident counts, and the host sees the scores -- plus the count matrix once, for the
features cache the reference writes next to the FASTA (scripts/phamer.py:132-134).  ``data_points`` keeps its
reference meaning (the normalised float64 matrix) but is materialised from the device only if somebody reads it;
assigning it (as phamer.score_points and the cross-validation do) switches the object to host rows, which are
scored through the float64-row entry point.

``phamer_scorer.both_strands`` (this project's own; `--both_strands`): every count row -- the two reference matrices
and the query contigs -- is folded with its reverse-complement permutation before it is normalised
(transform_kmers.fold_strands / phk_batch_fold_strands), so a contig scores bit for bit the same
whichever strand the assembler wrote.  The features cache always holds FORWARD counts: a run that starts from the cache
folds after loading it, so a cache is never folded twice and serves a forward-only run as well.

The k-means fit that yields the centroids is scikit-learn's, as in the reference (learning.kmeans); the density
method needs none (a dense float64 Gaussian kernel density per class, density.hip).  The svm method fits scikit-learn's
NuSVC() on the device (svm.hip) and scores 1.0 / 0.0 by its predict; dbscan clusters each class with learning.dbscan
(k-means when that finds fewer than three clusters) and scores with the kmeans method's nearest-centroid kernels.
The silhouette method raises NotImplementedError: the reference builds its negative side from the positive data
(scripts/phamer.py:295), so a faithful port scores 0 for every contig after an O((N + n)^2) silhouette pass
(SURVEY.md section 8).  The functional score_points keeps its method set (knn / kmeans / combo / density) and raises
for the others; score_with_scorer is the same call for every method of phamer_scorer.

The likelihood method (this project's own: likelihood.py) scores the contigs' integer COUNT rows
against the reference COUNT rows (``positive_counts`` / ``negative_counts``, which load_data() keeps beside the normalised
matrices when it is the scoring method); frequencies alone raise ValueError.

``phamer_scorer.predict_hosts`` / ``--hosts K`` (this project's own: hosts.py) ranks the negative
reference rows by the likelihood of each contig's count row and writes phamer_hosts.csv; it needs the same count rows
(``keep_reference_counts``) and leaves the scores as they are.
"""
import argparse
import logging
import os

import numpy as np

from . import _lib
from . import fileIO
from . import learning

logging.basicConfig(format='[%(asctime)s][%(levelname)s][%(funcName)s] - %(message)s')
logger = logging.getLogger(__name__)
logger.setLevel(logging.WARNING)

_GPU_METHODS = ('dbscan', 'knn', 'kmeans', 'combo', 'density', 'svm', 'likelihood')
_OTHER_METHODS = ('silhouette',)
_CENTROID_METHODS = ('kmeans', 'combo')
_FUNCTIONAL_METHODS = ('knn', 'kmeans', 'combo', 'density')   # what the functional score_points serves


def _lone(directory, suffixes, avoid_stem_suffix=None):
    """The file of `directory` the reference would pick (scripts/phamer.py:417-436): the only one with one of
    `suffixes`; among several, the first whose stem does not end in `avoid_stem_suffix`, else the first."""
    if not directory or not os.path.isdir(directory):
        return None
    names = [f for f in os.listdir(directory) if f.endswith(suffixes)]
    if not names:
        return None
    if len(names) > 1 and avoid_stem_suffix is None:
        return None
    for name in names:
        if len(names) == 1 or not os.path.splitext(name)[0].endswith(avoid_stem_suffix):
            return os.path.join(directory, name)
    return os.path.join(directory, names[0])


class phamer_scorer(object):

    def __init__(self):
        # where things are (scripts/phamer.py:46-57)
        self.input_directory = self.fasta_file = self.features_file = None
        self.data_directory = self.positive_features_file = self.negative_features_file = None
        self.output_directory = None
        # what the hot path reads (scripts/phamer.py:59-79)
        self.data_ids = None
        self.positive_ids = self.positive_data = None
        self.negative_ids = self.negative_data = None
        self.length_requirement = 5000
        self.scoring_method = 'combo'
        self.all_scoring_methods = ['dbscan', 'kmeans', 'knn', 'svm', 'density', 'silhouette', 'combo']
        self.method_function_map = dict(
            [(m, getattr(self, m + '_score_points')) for m in _GPU_METHODS] + [(m, self._outside_path) for m in _OTHER_METHODS])
        self.kmer_length = 4
        self.k_clusters = 86
        self.k_neighbors = 3
        self.both_strands = False           # fold every count row with its reverse complement (module docstring)
        self.positive_bandwidth = 0.005     # scripts/phamer.py:82-83 (density method)
        self.negative_bandwidth = 0.01
        self.svm_nu = 0.5                   # NuSVC()'s defaults (svm method); a table of other values: svm_grid.py
        self.svm_gamma = 'scale'
        self.pseudocount = 0.5              # likelihood method (this project's own, likelihood.py): the profiles' pseudocount,
        self.likelihood_per_kmer = False    # and whether a score is divided by its contig's k-mers
        self.positive_counts = self.negative_counts = None   # the reference COUNT rows, which that method scores against
        self.keep_reference_counts = False  # load_data() keeps them for any scoring method (predict_hosts needs them)
        self.k_clusters_positive = 86      # scripts/phamer.py:80-89 (dbscan method: its k-means fallback, eps, min_samples)
        self.k_clusters_negative = 20
        self.eps = [1, 1]
        self.min_samples = [2, 2]
        # t-SNE (scripts/phamer.py:66, 91-96); use_tsne_python and the plot are not ported
        self.tsne_data = None
        self.tsne_perplexity = 30.0
        self.early_exaggeration = 1.0
        self.tsne_init = "pca"
        self.tsne_learning_rate = 2000
        self.tsne_seed = 10
        self.pca_preprocess = True
        self.pca_preprocess_red = 50
        # centroids of the last kmeans / combo call (inspection, tests)
        self.positive_centroids = self.negative_centroids = None
        self.scores = None
        # query side: device-resident batch and / or host rows
        self._batch = None
        self._rows = None
        # host work that runs beside the path (main() only; the methods below are synchronous for API callers):
        # the features-cache write and the per-run k-means fit of the reference matrices
        self._defer_io = False
        self._pending_io = []
        self._centroid_future = None
        self._centroid_start = None

    # ---- data_points: the reference's attribute, lazily backed by the device batch --------------------
    @property
    def data_points(self):
        if self._rows is None and self._batch is not None:
            self._rows = self._batch.normalized()
        return self._rows

    @data_points.setter
    def data_points(self, rows):
        self._rows = rows
        self._drop_batch()

    def _drop_batch(self):
        if self._batch is not None:
            self._batch.close()
            self._batch = None

    # ---- files either side of the path ------------------------------------------------------------------
    def find_data_files(self):
        """Default reference files under the data directory (scripts/phamer.py:406-415)."""
        ref = os.path.join(self.data_directory, "reference_features")
        self.positive_features_file = os.path.join(ref, "positive_features.csv")
        self.negative_features_file = os.path.join(ref, "negative_features.csv")

    def find_input_files(self):
        """scripts/phamer.py:417-436: the FASTA (not the '*genes' one) and the lone features CSV of the input directory."""
        self.fasta_file = _lone(self.input_directory, ('.fasta', '.fa'), avoid_stem_suffix="genes") or self.fasta_file
        self.features_file = _lone(self.input_directory, ('.csv',)) or self.features_file

    def load_data(self, length_requirement=True):
        """Reference matrices (normalised) and the query contigs (scripts/phamer.py:103-142).  Queries come from the
        cached features CSV when the input directory has one; otherwise the FASTA is counted on the GPU, the counts are
        written through to ``<fasta>_features.csv`` and stay on the device for scoring.  A truthy
        ``length_requirement`` applies the length screen -- always with self.length_requirement (5000), as in the
        reference, whose CLI value is never forwarded."""
        self._load_reference()
        self._load_queries(length_requirement)

    def _load_reference(self):
        if self.scoring_method == 'likelihood' or self.keep_reference_counts:
            # the count rows are kept beside the normalised matrices (which are what the other branches make of the files)
            from . import kmer, transform_kmers
            fold = transform_kmers.fold_strands if self.both_strands else (lambda counts: counts)
            self.positive_ids, counts = fileIO.read_feature_file(self.positive_features_file, normalize=False)
            self.positive_counts = fold(counts)
            self.negative_ids, counts = fileIO.read_feature_file(self.negative_features_file, normalize=False)
            self.negative_counts = fold(counts)
            self.positive_data = kmer.normalize_counts(self.positive_counts)
            self.negative_data = kmer.normalize_counts(self.negative_counts)
            return
        self.positive_counts = self.negative_counts = None
        if self.both_strands:     # the counts are folded before they are normalised
            from . import kmer, transform_kmers
            self.positive_ids, counts = fileIO.read_feature_file(self.positive_features_file)
            self.positive_data = kmer.normalize_counts(transform_kmers.fold_strands(counts))
            self.negative_ids, counts = fileIO.read_feature_file(self.negative_features_file)
            self.negative_data = kmer.normalize_counts(transform_kmers.fold_strands(counts))
            return
        self.positive_ids, self.positive_data = fileIO.read_feature_file(self.positive_features_file, normalize=True)
        self.negative_ids, self.negative_data = fileIO.read_feature_file(self.negative_features_file, normalize=True)

    def _load_queries(self, length_requirement=True):
        self.find_input_files()
        lengths = None
        if self.features_file and os.path.exists(self.features_file):
            logger.info("Reading features from: %s..." % os.path.basename(self.features_file))
            from . import kmer
            self.data_ids, counts = fileIO.read_feature_file(self.features_file)
            _lap("features file read")
            # the cached counts go up once and the run scores from the same resident integers as a run that counted the
            # FASTA file (data_points, the reference's normalised float rows, is formed on demand); a file that is not an
            # integer k-mer count matrix keeps the reference's float rows
            self._drop_batch()
            self._rows = None
            batch = None
            if np.issubdtype(np.asarray(counts).dtype, np.integer) and np.asarray(counts).ndim == 2 and len(counts):
                batch = _lib.Batch.from_counts(_lib.get_context(), counts)
            if batch is not None:
                self._batch = batch
                self.kmer_length = int(round(np.log(batch.D) / np.log(4)))
                if self.both_strands:      # the cache holds forward counts: folded here, after loading, never in the file
                    batch.fold_strands()
            elif self.both_strands:
                from . import transform_kmers
                self.data_points = kmer.normalize_counts(transform_kmers.fold_strands(counts))
            else:
                self.data_points = kmer.normalize_counts(counts)
            del counts
            _lap("features on the device")
            self._start_pending_centroids()      # (beside the scan of the FASTA file for the length screen)
        elif self.fasta_file and os.path.exists(self.fasta_file):
            logger.info("Calculating features of: %s" % os.path.basename(self.fasta_file))
            lengths = self._count_fasta_on_device()
        else:
            raise SystemExit("No input fasta file or features file. Exiting...")
        if length_requirement:
            self.screen_by_length(_lengths=lengths)

    def _count_fasta_on_device(self):
        ctx = _lib.get_context()
        self._drop_batch()
        self._rows = None
        # the file is parsed straight into the upload's staging buffers (phk_batch_from_fasta_file): no host copy of the
        # sequences, nothing to free afterwards; the k-means thread starts beside it
        self._start_pending_centroids()
        fasta, self._batch = _lib.Fasta.count_file(ctx, self.fasta_file, self.kmer_length)
        _lap("FASTA parsed, uploaded, counted")
        try:
            self.data_ids = fasta.phamers_ids()
            lengths = fasta.lengths()
            counts = self._batch.counts_u32()
            _lap("counts on the host")
        finally:
            fasta.close()
        self.features_file = "{base}_features.csv".format(base=os.path.splitext(self.fasta_file)[0])
        ids, path = self.data_ids, self.features_file
        if self._defer_io:
            self._write_cache_async(counts, ids, path)
        else:
            fileIO.save_counts(counts, ids, path)
        if self.both_strands:      # after the forward counts have been taken for the cache
            self._batch.fold_strands()
        return lengths

    def _write_cache_async(self, counts, ids, path):
        """main(): the 0.6 s (1M contigs) of formatting and writing the features cache run beside the k-means fit and
        the scoring; the file appears under its name only when complete, and a failed write is raised by finish_io()."""
        import threading

        def write():
            tmp = path + ".part"
            try:
                _lap("features cache: write begins")
                fileIO.save_counts(counts, ids, tmp)
                _lap("features cache: written")
                os.replace(tmp, path)
            except BaseException as e:   # noqa: BLE001 -- handed to finish_io(), which raises it where the
                th.error = e             # reference's sequential save_counts would have
                try:
                    os.unlink(tmp)
                except OSError:
                    pass
        th = threading.Thread(target=write, name="phamers-features-cache")
        th.error = None
        th.start()
        self._pending_io.append(th)

    def finish_io(self):
        """Waits for file writes main() left running beside the scoring."""
        pending, self._pending_io = self._pending_io, []
        first = None
        for th in pending:
            th.join()
            first = first or getattr(th, "error", None)
        if first is not None:   # a failed write (disk full, read-only input directory) is an error of the run
            raise first

    def screen_by_length(self, length_requirement=None, _lengths=None):
        """Keep contigs of at least ``length_requirement`` bases (scripts/phamer.py:144-157): ids filtered on the host,
        rows by a device gather when the contigs are resident."""
        if length_requirement:
            self.length_requirement = length_requirement
        if _lengths is None:
            if not self.fasta_file or not os.path.exists(self.fasta_file):
                return
            from . import kmer
            fasta_ids, _lengths = kmer.fasta_lengths(self.fasta_file)
            _lap("FASTA indexed (ids, lengths)")
        else:
            fasta_ids = self.data_ids
        keep, long_ids = _length_screen(self.data_ids, fasta_ids, _lengths, self.length_requirement)
        _lap("length screen: rows matched")
        if keep is None:
            self.data_ids = np.asarray(self.data_ids)
            return      # every row is a long contig's own: nothing to drop (and 10^6 ids not sorted and copied, 0.4 s)
        if self._batch is not None:
            old, self._batch = self._batch, self._batch.select(np.flatnonzero(keep))
            old.close()
            self._rows = None if self._rows is None else self._rows[keep]
        elif self._rows is not None:
            self._rows = self._rows[keep]
        self.data_ids = long_ids      # (already a copy: boolean indexing)

    def get_phamer_output_filename(self):
        return os.path.join(self.output_directory, "phamer_scores.csv")

    def get_neighbors_output_filename(self):
        return os.path.join(self.output_directory, "phamer_neighbors.csv")

    def get_hosts_output_filename(self):
        return os.path.join(self.output_directory, "phamer_hosts.csv")

    def get_tsne_output_filename(self):
        """scripts/phamer.py:443-445."""
        return os.path.join(self.output_directory, "tsne_coordinates.csv")

    # ---- t-SNE (scripts/phamer.py:325-366) ---------------------------------------------------------------
    def do_tsne(self):
        """Embeds queries, positive and negative rows (in that order) into ``tsne_data`` (n, 2) on the device: PCA to
        ``pca_preprocess_red`` components when ``pca_preprocess``, then manifold.TSNE with the reference's parameters.
        ``data_points``, ``positive_data`` and ``negative_data`` stay as they were."""
        from . import manifold
        all_data = np.vstack((self.data_points, self.positive_data, self.negative_data))
        if self.pca_preprocess:
            logger.info("Pre-processing with PCA...")
            all_data = manifold.PCA(n_components=self.pca_preprocess_red).fit_transform(all_data)
        self.tsne_data = manifold.TSNE(perplexity=self.tsne_perplexity, early_exaggeration=self.early_exaggeration,
                                       random_state=self.tsne_seed, init=self.tsne_init,
                                       learning_rate=self.tsne_learning_rate).fit_transform(all_data)
        logger.info("t-SNE complete.")

    def save_tsne_data(self, args=None):
        """Writes ``tsne_data`` with the ids of the three row groups to get_tsne_output_filename()."""
        ids = np.concatenate((self.data_ids, self.positive_ids, self.negative_ids))
        chops = (len(self.data_ids), len(self.positive_ids), len(self.negative_ids))
        fileIO.save_tsne_data(self.get_tsne_output_filename(), self.tsne_data, ids, args=args, chops=chops)

    def make_summary_file(self, args=None):
        """phamer_scores.csv (scripts/phamer.py:316-323)."""
        self.phamer_output_filename = self.get_phamer_output_filename()
        fileIO.save_phamer_scores(self.data_ids, self.scores, self.phamer_output_filename, args=args)

    # ---- nearest references -------------------------------------------------------------------------------
    def find_nearest_references(self, k=5):
        """The k nearest reference rows of every contig among vstack(positive_data, negative_data), by (distance, index):
        sets ``neighbor_distances`` (n, k), ``neighbor_indices`` (n, k) into that stack and ``neighbor_ids`` (n, k) from
        ``positive_ids`` + ``negative_ids`` (None without them).  On the resident counts when there are any; ValueError
        for a contig without counts, as scoring raises."""
        model = _lib.Model(_lib.get_context(), self.positive_data, self.negative_data,
                           k_neighbors=min(self.k_neighbors, self.positive_data.shape[0] + self.negative_data.shape[0]))
        try:
            if self._batch is not None:
                dist, idx = self._batch.neighbors(model, k)
            else:
                q = np.asarray(self._rows, dtype=np.float64)
                if np.isnan(q).any():
                    raise ValueError("Input contains NaN.")
                dist, idx = model.neighbors(q, k)
        finally:
            model.close()
        self.neighbor_distances, self.neighbor_indices = dist, idx
        self.neighbor_ids = None
        if self.positive_ids is not None and self.negative_ids is not None:
            ids = np.concatenate((np.asarray(self.positive_ids, dtype=object), np.asarray(self.negative_ids, dtype=object)))
            self.neighbor_ids = ids[idx]
        return dist, idx

    def make_neighbors_file(self, args=None):
        """phamer_neighbors.csv beside phamer_scores.csv: one line per (contig, rank), see fileIO.save_phamer_neighbors."""
        idx = self.neighbor_indices
        ids = self.neighbor_ids
        if ids is None:
            n_pos = self.positive_data.shape[0]
            ids = np.where(idx < n_pos, "positive_", "negative_").astype(object) + np.where(idx < n_pos, idx, idx - n_pos).astype(str).astype(object)
        self.neighbors_output_filename = self.get_neighbors_output_filename()
        fileIO.save_phamer_neighbors(self.neighbors_output_filename, self.data_ids, ids, idx < self.positive_data.shape[0],
                                     self.neighbor_distances, args=args)

    # ---- host prediction (this project's own: hosts.py) -----------------------------
    def predict_hosts(self, top=5, model='markov'):
        """The ``top`` rows of ``negative_counts`` (the bacterial genomes) every contig is most likely to come from, by the
        likelihood of its count row under each row's ``model`` table (hosts.py), annotated with the z-score and p-value of
        the per-k-mer log-likelihood under a null fitted on ``positive_counts`` (the phage genomes -- all of them, see
        hosts.predict).  Sets ``host_indices`` (n, top) into the negative rows, ``host_ids`` (n, top; from
        ``negative_ids``, or 'negative_<row>' without them), ``host_log_likelihood``, ``host_per_kmer``, ``host_z`` and
        ``host_p_value``.  On the resident counts when there are any; with ``both_strands`` both sides are the folded rows,
        as for the likelihood method.  The ValueErrors of likelihood_score_points when count rows are missing."""
        from . import hosts
        ref = self.positive_counts, self.negative_counts
        if any(c is None for c in ref) or any(d is not None and len(d) != len(c)
                                              for c, d in zip(ref, (self.positive_data, self.negative_data))):
            raise ValueError("host prediction needs the reference COUNT rows (positive_counts / negative_counts, which "
                             "load_data() reads from the feature files when keep_reference_counts is set or the scoring "
                             "method is 'likelihood'): positive_data / negative_data hold frequencies only")
        if self._batch is None:
            raise ValueError("host prediction needs the contigs' integer k-mer counts (a counted FASTA file or an "
                             "integer features file): data_points holds frequencies only")
        top = _lib.check_hosts_top(top, len(ref[1]))
        table = _lib.HostTable(_lib.get_context(), hosts._table(ref[1], model, self.pseudocount))
        try:
            null = table.null_fit(hosts._count_rows(ref[0], "positive_counts"))
            idx, S = self._batch.hosts(table, top)
        finally:
            table.close()
        r = hosts._annotate(idx, S, self._batch.row_sums(), null)
        self.host_indices, self.host_log_likelihood, self.host_per_kmer = r.indices, r.log_likelihood, r.per_kmer
        self.host_z, self.host_p_value = r.z, r.p_value
        if self.negative_ids is not None:
            self.host_ids = np.asarray(self.negative_ids, dtype=object)[idx]
        else:
            self.host_ids = "negative_" + idx.astype(str).astype(object)
        return r

    def make_hosts_file(self, args=None):
        """phamer_hosts.csv beside phamer_scores.csv: one line per (contig, rank), see fileIO.save_phamer_hosts."""
        self.hosts_output_filename = self.get_hosts_output_filename()
        fileIO.save_phamer_hosts(self.hosts_output_filename, self.data_ids, self.host_ids, self.host_log_likelihood,
                                 self.host_per_kmer, self.host_z, self.host_p_value, args=args)

    # ---- scoring ------------------------------------------------------------------------------------------
    def equalize_reference_data(self):
        """The FIRST min(n+, n-) rows of each class (scripts/phamer.py:159-175)."""
        m = min(self.positive_data.shape[0], self.negative_data.shape[0])
        if self.positive_data.shape[0] != self.negative_data.shape[0]:
            logger.debug("Equalizing reference data to: %d data points" % m)
            self.positive_data, self.negative_data = self.positive_data[:m], self.negative_data[:m]
            self.positive_ids = None if self.positive_ids is None else self.positive_ids[:m]
            self.negative_ids = None if self.negative_ids is None else self.negative_ids[:m]
            if self.positive_counts is not None and self.negative_counts is not None:
                self.positive_counts, self.negative_counts = self.positive_counts[:m], self.negative_counts[:m]
            self.num_positive = self.num_negative = m

    def score_points(self):
        """Scores the query contigs against ``positive_data`` / ``negative_data`` with ``scoring_method``
        (scripts/phamer.py:177-195)."""
        self.num_points = self._batch.n if self._batch is not None else self.data_points.shape[0]
        self.num_positive, self.num_negative = self.positive_data.shape[0], self.negative_data.shape[0]
        logger.debug("Scoring %d points. Method: %s..." % (self.num_points, self.scoring_method))
        self.scores = np.array(self.method_function_map[self.scoring_method]())
        return self.scores

    def _outside_path(self):
        raise NotImplementedError("scoring method %r is not available: the reference's silhouette method scores its "
                                  "contigs against the positive data twice (scripts/phamer.py:295), i.e. 0 for every "
                                  "contig; dbscan / kmeans / knn / svm / density / combo are available"
                                  % (self.scoring_method,))

    def _centroids_of(self, pos, neg, k_clusters, deliver=None):
        """k-means labels -> the reference's per-label means, for both classes.  deliver: called from a helper thread,
        which gets a device context of its own (a context is not shared between threads) and hands the result (or the
        exception) to this Future BEFORE it closes that context -- freeing the context's buffers waits for the device,
        0.2 s beside the main thread's upload."""
        _lap("k-means: begin")
        ctx = None
        try:
            try:
                # (inside the guarded block: a context that cannot be created -- no memory for its streams, a HIP error --
                # must reach the Future as an exception, or the main thread waits for this result for ever)
                ctx = _lib.Context(_lib.default_device()) if deliver is not None else None
                out = []
                for d in (pos, neg):
                    out.append(learning.get_centroids(d, learning.kmeans(d, k_clusters, _ctx=ctx)))
                    _lap("k-means: one class done")
                out = tuple(out)
            except BaseException as e:   # noqa: BLE001 -- raised again by Future.result() in the main thread
                if deliver is None:
                    raise
                deliver.set_exception(e)
                return None
            if deliver is not None:
                deliver.set_result(out)
            return out
        finally:
            if ctx is not None:
                ctx.close()

    def prefetch_centroids(self, after_fasta_read=False):
        """Starts the k-means fit of the reference matrices as they are NOW on a helper thread, so that it runs beside the
        upload, the counting and the cache write (the seeding's matrix products release the GIL; the Lloyd sweeps run on
        the device through a context of the thread's own); _fit_centroids takes the result if the matrices have not been
        replaced since, and fits afresh otherwise.  after_fasta_read: the thread starts when the FASTA file has been
        parsed -- beside the native reader's threads it took the parse from 0.32 to 0.48 s (1M contigs) and gained
        nothing, since the fit (0.11 s) fits beside what follows."""
        if os.environ.get("PHAMERS_KMEANS", "device") == "gpu":
            return
        pos, neg, k = self.positive_data, self.negative_data, self.k_clusters

        def start():
            import threading
            from concurrent.futures import Future
            fut = Future()
            self._centroid_future = (pos, neg, k, fut)
            threading.Thread(target=self._centroids_of, args=(pos, neg, k, fut), name="phamers-kmeans").start()
        if after_fasta_read and os.environ.get("PHAMERS_KMEANS_START", "after_read") != "early":
            self._centroid_start = start      # _count_fasta_on_device() calls it once the file is parsed
        else:
            start()

    def _start_pending_centroids(self):
        start, self._centroid_start = self._centroid_start, None
        if start is not None:
            start()

    def _fit_centroids(self):
        """k-means with k_clusters on each class, then the cluster means (scripts/phamer.py:245-248)."""
        self._centroid_start = None       # (never started: no FASTA was read -- fit here, in the main thread's context)
        fut, self._centroid_future = self._centroid_future, None
        if fut is not None and fut[0] is self.positive_data and fut[1] is self.negative_data and fut[2] == self.k_clusters:
            self.positive_centroids, self.negative_centroids = fut[3].result()
            return
        self.positive_centroids, self.negative_centroids = self._centroids_of(self.positive_data, self.negative_data,
                                                                              self.k_clusters)

    def _gpu_score(self, method, centroids=None):
        with_centroids = method in _CENTROID_METHODS
        if with_centroids and centroids is None:
            self._fit_centroids()
            centroids = self.positive_centroids, self.negative_centroids
        model = _lib.Model(_lib.get_context(), self.positive_data, self.negative_data,
                           centroids[0] if with_centroids else None,
                           centroids[1] if with_centroids else None, k_neighbors=self.k_neighbors)
        try:
            if method == 'density':
                model.set_bandwidths(self.positive_bandwidth, self.negative_bandwidth)
            elif method == 'svm':
                model.fit_svm(self.svm_nu, self.svm_gamma)        # NuSVC() defaults: nu 0.5, gamma 'scale', tol 1e-3
            if self._batch is not None:
                return self._batch.score(model, method)          # resident counts; NaN rows raise ValueError
            q = np.asarray(self._rows, dtype=np.float64)
            if np.isnan(q).any():
                raise ValueError("Input contains NaN.")           # what scikit-learn raises for the reference
            return model.score(q, method)
        finally:
            model.close()

    def knn_score_points(self):
        """scripts/phamer.py:268-273."""
        return self._gpu_score('knn')

    def kmeans_score_points(self):
        """scripts/phamer.py:240-256: tanh proximity metric to the nearest centroid of each class."""
        return self._gpu_score('kmeans')

    def dbscan_score_points(self):
        """scripts/phamer.py:212-238: DBSCAN per class (eps / min_samples), k-means with k_clusters_positive /
        k_clusters_negative for a class where DBSCAN's largest label is below 2, the clusters' means (noise excluded), then
        the kmeans method's proximity metric to the nearest centroid of each class.  A list of one-element lists, as the
        reference returns (score_points makes it an (n, 1) array)."""
        pos, neg = self.positive_data, self.negative_data
        positive_assignment = learning.dbscan(pos, self.eps[0], self.min_samples[0])
        negative_assignment = learning.dbscan(neg, self.eps[1], self.min_samples[1])
        if max(positive_assignment) < 2:
            logger.warning("Clustering positive with k-means instead...")
            positive_assignment = learning.kmeans(pos, self.k_clusters_positive)
        if max(negative_assignment) < 2:
            logger.warning("Clustering negative with k-means instead...")
            negative_assignment = learning.kmeans(neg, self.k_clusters_negative)
        centroids = (learning.get_centroids(pos, positive_assignment), learning.get_centroids(neg, negative_assignment))
        self.positive_centroids, self.negative_centroids = centroids
        return [[s] for s in self._gpu_score('kmeans', centroids)]

    def svm_score_points(self):
        """scripts/phamer.py:258-266: NuSVC().fit(vstack(positive, negative), labels 1 / 0).predict(points) -- the fit and
        the prediction on the device (svm.hip), 1.0 / 0.0 per contig."""
        return self._gpu_score('svm')

    def density_score_points(self):
        """scripts/phamer.py:275-287: log-density under the positive class minus that under the negative class (Gaussian
        kernels of width positive_bandwidth / negative_bandwidth; learning.get_density per class)."""
        return self._gpu_score('density')

    def combo_score_points(self):
        """scripts/phamer.py:303-313: knn score + kmeans score (one fused GPU pass)."""
        return self._gpu_score('combo')

    def likelihood_score_points(self):
        """This project's own method (likelihood.py): the log-likelihood ratio, in nats, of the contig's integer count row
        under the two classes' mixtures of multinomials -- ``pseudocount`` smooths the reference profiles,
        ``likelihood_per_kmer`` divides by the contig's k-mers.  It scores counts: the resident batch (a counted FASTA
        file or an integer features cache) against ``positive_counts`` / ``negative_counts``, which load_data() keeps
        when this is the scoring method.  ValueError when only frequencies are there."""
        from . import likelihood
        ref = self.positive_counts, self.negative_counts
        if any(c is None for c in ref) or any(d is not None and len(d) != len(c)
                                              for c, d in zip(ref, (self.positive_data, self.negative_data))):
            raise ValueError("scoring method 'likelihood' needs the reference COUNT rows (positive_counts / negative_counts, "
                             "which load_data() reads from the feature files when it is the scoring method): "
                             "positive_data / negative_data hold frequencies only")
        if self._batch is None:
            raise ValueError("scoring method 'likelihood' needs the contigs' integer k-mer counts (a counted FASTA file or an "
                             "integer features file): data_points holds frequencies only")
        table = _lib.LikelihoodTable(_lib.get_context(), likelihood.log_table(ref[0], self.pseudocount),
                                     likelihood.log_table(ref[1], self.pseudocount))
        try:
            scores = self._batch.likelihood(table)
        finally:
            table.close()
        if self.likelihood_per_kmer:
            with np.errstate(invalid='ignore', divide='ignore'):
                scores = scores / self._batch.row_sums().astype(np.float64)
        return scores


def _length_screen(data_ids, fasta_ids, lengths, length_requirement):
    """The rows screen_by_length keeps (scripts/phamer.py:144-157): (keep mask over data_ids, ids of the long contigs), or
    (None, None) when every row is a long contig's own and nothing is dropped."""
    is_long = np.asarray(lengths) >= length_requirement
    # the rows are the file's records in the file's order: always so when they were just counted from it, and the
    # usual case when they came from the features cache written beside it (one vectorised comparison to know)
    own_rows = fasta_ids is data_ids or (
        len(fasta_ids) == len(data_ids) and bool(np.array_equal(np.asarray(fasta_ids), np.asarray(data_ids))))
    if own_rows and is_long.all():
        return None, None
    long_ids = np.asarray(fasta_ids)[is_long]
    if own_rows:
        # the reference keeps a row when its id is that of SOME contig long enough (np.in1d): true for every long contig's
        # own row, so only the short contigs' ids have to be looked up (none on a batch of long contigs; a sort of 10^6
        # strings otherwise, 0.2 s)
        keep = is_long.copy()
        short = ~is_long
        if short.any() and is_long.any():
            keep[short] = np.isin(np.asarray(data_ids)[short], long_ids)
    else:
        keep = np.isin(data_ids, long_ids)
    return keep, long_ids


def score_points(scoring_data, positive_training_data, negative_training_data, method=None):
    """Functional form of phamer_scorer.score_points (scripts/phamer.py:451-468), the scoring function of the
    reference's cross-validation (scripts/cross_validate.py:95), for the methods it has always served: knn / kmeans /
    combo / density.  The others raise NotImplementedError before any device work, as before; svm and dbscan are
    served by phamer_scorer.score_points, by cross_validator (which routes them itself) and by score_with_scorer."""
    method = method or phamer_scorer().scoring_method
    if method not in _FUNCTIONAL_METHODS:
        raise NotImplementedError("score_points(method=%r): the functional form scores %s; use phamer_scorer.score_points "
                                  "or score_with_scorer for dbscan / svm" % (method, " / ".join(_FUNCTIONAL_METHODS)))
    return score_with_scorer(scoring_data, positive_training_data, negative_training_data, method)


def score_with_scorer(scoring_data, positive_training_data, negative_training_data, method=None):
    """The body of the reference's functional score_points (scripts/phamer.py:451-468) for every method phamer_scorer
    has: a scorer over the given matrices, then its score_points()."""
    scorer = phamer_scorer()
    scorer.scoring_method = method or scorer.scoring_method
    scorer.data_points = scoring_data
    scorer.positive_data, scorer.negative_data = positive_training_data, negative_training_data
    return scorer.score_points()


def score_contigs(sequences, positive_training_data, negative_training_data, kmer_length=4, method='combo', both_strands=False,
                  k_clusters=None):
    """Count -> normalise -> score a list of contig strings, device resident (what load_data + score_points do for a
    FASTA input, scripts/phamer.py:131,139,579).  ``both_strands``: the contigs' counts are folded with their reverse
    complement on the device before scoring; the training data are taken as given -- pass matrices normalised from
    folded counts (transform_kmers.fold_strands).  ``k_clusters``: clusters per class of the kmeans / combo fit (default:
    phamer_scorer's 86)."""
    scorer = phamer_scorer()
    scorer.scoring_method = method
    if k_clusters is not None:
        scorer.k_clusters = int(k_clusters)
    scorer.kmer_length = kmer_length
    scorer.both_strands = bool(both_strands)
    scorer._batch = _lib.Batch.from_sequences(_lib.get_context(), list(sequences), kmer_length)
    if both_strands:
        scorer._batch.fold_strands()
    scorer.positive_data, scorer.negative_data = positive_training_data, negative_training_data
    try:
        return scorer.score_points()
    finally:
        scorer._drop_batch()


_clock0 = [None]


def _lap(what):
    """--debug: seconds since main() began, from whichever thread."""
    import time
    if _clock0[0] is not None:
        logger.debug("%-34s %.3f s" % (what, time.perf_counter() - _clock0[0]))


def main(argv=None):
    """The reference's command line for this path (scripts/phamer.py:512-598), cut to what the path uses:
        python -m phamers_amd.phamer -in <input_dir> -data <data_dir> [--equalize_reference]
    Scores go to <input_dir>/phamer_output/phamer_scores.csv (or -out).  As in the reference the method is always
    'combo' (its --method is parsed and never applied) -- unless --pseudocount or --per_kmer, this
    project's own flags, select the likelihood method (likelihood.py)."""
    ap = _parser()
    args = ap.parse_args(argv)
    if args.do_tsne or args.plot_tsne:
        raise NotImplementedError("t-SNE / plots (-do_tsne, -plot) are outside the accelerated path (SURVEY.md section 8)")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if hasattr(args, "neighbors"):
        if not 1 <= args.neighbors <= _lib.NEIGHBORS_MAX_K:
            ap.error("--neighbors must be in 1..%d (got %d)" % (_lib.NEIGHBORS_MAX_K, args.neighbors))
        if (args.gpus and args.gpus > 1) or world > 1 or os.environ.get("PHAMERS_FORCE_RANK_PATH") == "1":
            ap.error("--neighbors is not sharded: run it on one GPU (without --gpus)")
    if hasattr(args, "hosts") or hasattr(args, "hosts_model"):
        if not hasattr(args, "hosts"):
            ap.error("--hosts_model needs --hosts K")
        if not 1 <= args.hosts <= _lib.HOSTS_MAX_TOP:
            ap.error("--hosts must be in 1..%d (got %d)" % (_lib.HOSTS_MAX_TOP, args.hosts))
        if (args.gpus and args.gpus > 1) or world > 1 or os.environ.get("PHAMERS_FORCE_RANK_PATH") == "1":
            ap.error("--hosts is not sharded: run it on one GPU (without --gpus)")
    if (hasattr(args, "pseudocount") or hasattr(args, "per_kmer")) and (
            (args.gpus and args.gpus > 1) or world > 1 or os.environ.get("PHAMERS_FORCE_RANK_PATH") == "1"):
        ap.error("--pseudocount / --per_kmer (the likelihood method) are not sharded: run them on one GPU (without --gpus)")
    if world > 1 or os.environ.get("PHAMERS_FORCE_RANK_PATH") == "1":   # one rank of a sharded run (started below, or by
                                                                        # torch.distributed.run; forced: a 1-rank group, tests)
        return _run_rank(ap, args)
    if args.gpus and args.gpus > 1:    # the launcher: it never touches the GPU itself -- the ranks are its children
        import sys
        from . import dist as pdist
        cmd = [sys.executable, "-m", "phamers_amd.phamer"] + list(sys.argv[1:] if argv is None else argv)
        rc = pdist.launch_ranks(args.gpus, cmd, require_gpus=os.environ.get("PHAMERS_DIST_BACKEND", "nccl") == "nccl")
        if rc:
            raise SystemExit(rc)
        return None
    return _run(ap, args)


def _parser():
    ap = argparse.ArgumentParser(description='This script scores contigs based on feature similarity',
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    for flags, kw in (
            (('-in', '--input_directory'), dict(help='Directory containing input files')),
            (('-fasta', '--fasta_file'), dict(help='Fasta compilation file of unknown sequences')),
            (('-features', '--features_file'), dict(help='Input feature file')),
            (('-data', '--data_directory'), dict(help='Directory containing reference_features/')),
            (('-pf', '--positive_features'), dict(help='Positive reference features CSV')),
            (('-nf', '--negative_features'), dict(help='Negative reference features CSV')),
            (('-out', '--output_directory'), dict(help='Output directory path')),
            (('-k', '--kmer_length'), dict(type=int, default=4, help='k-mer length')),
            (('-l', '--length_requirement'), dict(type=int, default=5000, help='Input sequence length requirement')),
            (('-equal', '-e', '--equalize_reference'), dict(action='store_true', help='Same number of reference points')),
            (('--gpus',), dict(type=int, default=1, help='GPUs of this node to shard the contigs over (one process per GPU)')),
            (('--both_strands',), dict(action='store_true', help='Fold every count row with its reverse complement: a contig '
                                                                 'scores the same on either strand')),
            # (no default: without the flag the attribute is absent, and the argument summary stamped into the output
            # files is what it was)
            (('--neighbors',), dict(type=int, default=argparse.SUPPRESS, metavar='K',
                                    help='Also write phamer_neighbors.csv: the K nearest reference rows of every contig '
                                         '(1..28; one GPU only)')),
            # (long options only: -k is the k-mer length.  No default, as --neighbors: absent, the scorer keeps its own)
            (('--k_neighbors',), dict(type=int, default=argparse.SUPPRESS, metavar='K',
                                      help="Neighbours of the k-NN vote (the scorer's default: 3; combo_grid.py tables others)")),
            (('--k_clusters',), dict(type=int, default=argparse.SUPPRESS, metavar='K',
                                     help="Clusters per class of the k-means fit (the scorer's default: 86)")),
            # (no defaults either: the method stays 'combo' unless one of the two is given, and the stamped summary is unchanged)
            (('--pseudocount',), dict(type=float, default=argparse.SUPPRESS, metavar='A',
                                      help="Score with the likelihood method (likelihood.py), the reference profiles smoothed "
                                           "by this pseudocount (the scorer's default: 0.5; one GPU only)")),
            (('--per_kmer',), dict(action='store_true', default=argparse.SUPPRESS,
                                   help="Score with the likelihood method, every score divided by its contig's k-mers")),
            # (no defaults, as --neighbors: the stamped summary of phamer_scores.csv is what a run without them writes)
            (('--hosts',), dict(type=int, default=argparse.SUPPRESS, metavar='K',
                                help='Also write phamer_hosts.csv: the K negative reference rows (bacterial genomes) every '
                                     'contig is most likely to come from, with z-score and p-value under a null fitted on '
                                     'the positive rows (hosts.py; 1..16; one GPU only)')),
            (('--hosts_model',), dict(choices=('markov', 'multinomial'), default=argparse.SUPPRESS,
                                      help="Log table of --hosts (default: markov, a chain of order k - 1 per genome)")),
            (('-v', '--verbose'), dict(action='store_true')),
            (('--debug',), dict(action='store_true')),
            # the rest of the reference's command line (scripts/phamer.py:515-553), so that its launch scripts
            # (run.sh, submit/*.sh) parse unchanged.  The reference parses --method / --eps / --minPts and never applies
            # them (the method is always 'combo'); t-SNE, plots and counting the reference sets from FASTA are outside
            # the accelerated path and are refused when asked for.
            (('-tsne', '--tsne_file'), dict(help='(outside the accelerated path)')),
            (('-p', '--positive_fasta'), dict(help='(outside the accelerated path: give -pf)')),
            (('-n', '--negative_fasta'), dict(help='(outside the accelerated path: give -nf)')),
            (('-id', '--file_identifier'), dict(default='.fna', help='(used with -n only)')),
            (('-do_tsne', '--do_tsne'), dict(action='store_true', help='(outside the accelerated path)')),
            (('-pxty', '--perplexity'), dict(type=float, default=30, help='(t-SNE only)')),
            (('-plot', '--plot_tsne'), dict(action='store_true', help='(outside the accelerated path)')),
            (('-m', '--method'), dict(default='combo', help='parsed and, as in the reference, not applied')),
            (('-eps', '--eps'), dict(type=float, default=2.1, help='parsed and, as in the reference, not applied')),
            (('-mp', '--minPts'), dict(type=int, default=2, help='parsed and, as in the reference, not applied'))):
        ap.add_argument(*flags, **kw)
    return ap


def _apply_k_options(scorer, args):
    """--k_neighbors / --k_clusters, where given, onto the scorer's attributes of those names."""
    for name in ("k_neighbors", "k_clusters"):
        if hasattr(args, name):
            if getattr(args, name) < 1:
                raise SystemExit("--%s must be >= 1 (got %d). Exiting..." % (name, getattr(args, name)))
            setattr(scorer, name, getattr(args, name))


def _apply_likelihood_options(scorer, args):
    """--pseudocount / --per_kmer: either one selects the likelihood method and sets the scorer's attribute."""
    if hasattr(args, "pseudocount"):
        if not (np.isfinite(args.pseudocount) and args.pseudocount > 0):
            raise SystemExit("--pseudocount must be finite and > 0 (got %r). Exiting..." % (args.pseudocount,))
        scorer.pseudocount = args.pseudocount
    if hasattr(args, "per_kmer"):
        scorer.likelihood_per_kmer = True
    if hasattr(args, "pseudocount") or hasattr(args, "per_kmer"):
        scorer.scoring_method = 'likelihood'


def _run(ap, args):
    logger.setLevel(logging.DEBUG if args.debug else logging.INFO if args.verbose else logging.WARNING)

    scorer = phamer_scorer()
    scorer.kmer_length = args.kmer_length
    scorer.both_strands = args.both_strands
    _apply_k_options(scorer, args)
    _apply_likelihood_options(scorer, args)
    hosts_top, hosts_model = getattr(args, "hosts", None), getattr(args, "hosts_model", "markov")
    scorer.keep_reference_counts = hosts_top is not None
    scorer.input_directory, scorer.fasta_file, scorer.features_file = args.input_directory, args.fasta_file, args.features_file
    if args.data_directory:
        scorer.data_directory = args.data_directory
        scorer.find_data_files()
    scorer.positive_features_file = args.positive_features or scorer.positive_features_file
    scorer.negative_features_file = args.negative_features or scorer.negative_features_file
    if not (scorer.positive_features_file and scorer.negative_features_file):
        ap.error("give -data <dir with reference_features/> or -pf and -nf")
    scorer.output_directory = args.output_directory or os.path.join(
        args.input_directory or os.path.dirname(args.fasta_file or args.features_file or '.'), "phamer_output")
    # load_data(), with the host work that does not depend on the contigs started early: the reference matrices are
    # read (and equalised) first, their k-means fit runs beside the FASTA ingest and the counting, and the features
    # cache is written beside the scoring.  Same files, same numbers as the sequential order of the reference.
    import time
    _clock0[0] = time.perf_counter()
    lap = _lap
    scorer._defer_io = True
    try:
        scorer._load_reference()
        if args.equalize_reference:
            scorer.equalize_reference_data()
        lap("reference matrices")
        if scorer.scoring_method != 'likelihood':     # (which fits nothing)
            scorer.prefetch_centroids(after_fasta_read=True)
        scorer._load_queries(args.length_requirement)
        lap("contigs counted")
        os.makedirs(scorer.output_directory, exist_ok=True)
        scorer.score_points()
        lap("scored")
        neighbors = getattr(args, "neighbors", None)
        if neighbors is not None:      # the scores file is stamped as a run without the flag stamps it
            args = argparse.Namespace(**{k: v for k, v in vars(args).items() if k != "neighbors"})
        if hosts_top is not None:
            hosts_given = {k: v for k, v in vars(args).items() if k in ("hosts", "hosts_model")}
            args = argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in hosts_given})
        scorer.make_summary_file(args=args)
        lap("scores written")
        if neighbors is not None:
            scorer.find_nearest_references(neighbors)
            lap("nearest references found")
            scorer.make_neighbors_file(args=argparse.Namespace(neighbors=neighbors, **vars(args)))
            lap("nearest references written")
        if hosts_top is not None:
            scorer.predict_hosts(hosts_top, hosts_model)
            lap("hosts ranked")
            scorer.make_hosts_file(args=argparse.Namespace(**dict(vars(args), **hosts_given)))
            lap("hosts written")
    finally:
        scorer.finish_io()
        lap("features cache complete")
    return scorer


def _rank_count_and_score(fasta_file, part, kmer_length, method, positive, negative, cpos, cneg, k_neighbors, keep_of, gpu,
                          both_strands=False):
    """One rank's share of the FASTA file on its GPU: the records that begin in byte range ``part`` = (rank, world) are parsed
    straight into the upload's staging buffers (phk_batch_from_fasta_part), counted, screened (``keep_of(ids, lengths)`` ->
    boolean mask over this rank's records, decided with every rank's ids) and scored.  Returns (ids, counts uint32 of every
    record, keep mask, scores of the kept).  ``both_strands``: the rank folds its own rows after the forward counts have
    been taken for the cache; nothing more is exchanged.  (A module-level function so that the CPU tests can put the oracle in its
    place: the product has no CPU path.)"""
    ctx = _lib.get_context(gpu)
    threads = max(1, (os.cpu_count() or 1) // max(1, part[1]))
    fasta, batch = _lib.Fasta.count_file(ctx, fasta_file, kmer_length, threads=threads, part=part)
    try:
        ids, lengths = fasta.phamers_ids(), fasta.lengths()
    finally:
        fasta.close()
    try:
        counts = batch.counts_u32() if batch.n else np.zeros((0, 4 ** int(kmer_length)), dtype=np.uint32)
        keep = keep_of(ids, lengths)
        scores = np.zeros(0)
        if keep.any():
            sub = batch if keep.all() else batch.select(np.flatnonzero(keep))
            if both_strands:
                sub.fold_strands()
            cen = method in _CENTROID_METHODS
            model = _lib.Model(ctx, positive, negative, cpos if cen else None, cneg if cen else None, k_neighbors=k_neighbors)
            try:
                if method == 'svm':
                    model.fit_svm()
                scores = sub.score(model, method)
            finally:
                model.close()
                if sub is not batch:
                    sub.close()
        return ids, counts, keep, scores
    finally:
        batch.close()


def _run_rank(ap, args):
    """One rank of `python -m phamers_amd.phamer ... --gpus N` (scripts/phamer.py:512-598 on a shard): the
    reference matrices and centroids are replicated, every rank loads, counts and scores the records of ITS byte range of the
    FASTA file, and the ranks exchange ids, lengths (for the length screen, which looks ids up across the whole file), scores
    and -- for the features cache rank 0 writes -- counts.  Rank 0 writes the same phamer_scores.csv and <fasta>_features.csv
    as the one-GPU run, byte for byte."""
    import torch
    import torch.distributed as tdist
    from . import dist as pdist
    logger.setLevel(logging.DEBUG if args.debug else logging.INFO if args.verbose else logging.WARNING)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    backend = os.environ.get("PHAMERS_DIST_BACKEND", "nccl")
    gpu = None
    if backend == "nccl":
        gpu = pdist.rank_device()
        tdist.init_process_group("nccl", device_id=torch.device("cuda", gpu))
    else:
        tdist.init_process_group(backend)
    dev = torch.device("cuda", gpu) if backend == "nccl" else torch.device("cpu")
    try:
        scorer = phamer_scorer()
        scorer.kmer_length = args.kmer_length
        scorer.both_strands = args.both_strands
        _apply_k_options(scorer, args)
        scorer.input_directory, scorer.fasta_file, scorer.features_file = args.input_directory, args.fasta_file, args.features_file
        if args.data_directory:
            scorer.data_directory = args.data_directory
            scorer.find_data_files()
        scorer.positive_features_file = args.positive_features or scorer.positive_features_file
        scorer.negative_features_file = args.negative_features or scorer.negative_features_file
        if not (scorer.positive_features_file and scorer.negative_features_file):
            ap.error("give -data <dir with reference_features/> or -pf and -nf")
        scorer.output_directory = args.output_directory or os.path.join(
            args.input_directory or os.path.dirname(args.fasta_file or args.features_file or '.'), "phamer_output")
        scorer.find_input_files()
        if not (scorer.fasta_file and os.path.exists(scorer.fasta_file)):
            raise SystemExit("--gpus needs the input FASTA file (a features cache alone is scored by one GPU). Exiting...")
        scorer._load_reference()
        if args.equalize_reference:
            scorer.equalize_reference_data()
        # centroids: fitted once, by rank 0, and handed to every rank (the fit is deterministic; this makes "replicated" literal)
        shape = (scorer.k_clusters, scorer.positive_data.shape[1])
        cen = torch.zeros((2,) + shape, dtype=torch.float64, device=dev)
        if rank == 0:
            scorer._fit_centroids()
            cen[0] = torch.from_numpy(np.ascontiguousarray(scorer.positive_centroids)).to(dev)
            cen[1] = torch.from_numpy(np.ascontiguousarray(scorer.negative_centroids)).to(dev)
        tdist.broadcast(cen, src=0)
        cpos, cneg = cen[0].cpu().numpy(), cen[1].cpu().numpy()

        screen = int(scorer.length_requirement) if args.length_requirement else 0   # (the CLI value is a switch, as in the reference)

        def keep_of(ids, lengths):
            # the screen keeps a row whose id is that of SOME contig long enough, anywhere in the file: decided on every
            # rank from all ranks' ids and lengths, exactly as the one-GPU run decides it
            everything = [None] * world
            tdist.all_gather_object(everything, (list(ids), np.asarray(lengths, dtype=np.int64)))
            keep_of.all_ids = np.array([x for part in everything for x in part[0]], dtype=object if any(
                x is None for part in everything for x in part[0]) else None)
            if keep_of.all_ids.dtype != object:
                keep_of.all_ids = keep_of.all_ids.astype(str)
            all_len = np.concatenate([part[1] for part in everything]) if everything else np.zeros(0, dtype=np.int64)
            first = sum(len(part[0]) for part in everything[:rank])
            keep_of.kept_ids = keep_of.all_ids
            keep_of.all_keep = np.ones(len(all_len), dtype=bool)
            if screen:
                k_all, long_ids = _length_screen(keep_of.all_ids, keep_of.all_ids, all_len, screen)
                if k_all is not None:    # (rows and ids exactly as screen_by_length leaves them in the one-GPU run)
                    keep_of.all_keep, keep_of.kept_ids = k_all, long_ids
            return keep_of.all_keep[first:first + len(ids)]

        strands = {"both_strands": True} if scorer.both_strands else {}
        ids, counts, keep, scores = _rank_count_and_score(scorer.fasta_file, (rank, world), scorer.kmer_length, scorer.scoring_method,
                                                          scorer.positive_data, scorer.negative_data, cpos, cneg, scorer.k_neighbors,
                                                          keep_of, gpu, **strands)
        all_scores = pdist.gather_variable(torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float64)).to(dev)).cpu().numpy()
        all_counts = pdist.gather_rows_to_root(torch.from_numpy(np.ascontiguousarray(counts).view(np.int32)).to(dev))
        if rank == 0:
            os.makedirs(scorer.output_directory, exist_ok=True)
            scorer.data_ids = keep_of.kept_ids
            scorer.scores = all_scores
            scorer.make_summary_file(args=args)
            cache = "{base}_features.csv".format(base=os.path.splitext(scorer.fasta_file)[0])
            fileIO.save_counts(all_counts.cpu().numpy().view(np.uint32), keep_of.all_ids, cache)
        tdist.barrier()
        return scorer if rank == 0 else None
    finally:
        tdist.destroy_process_group()


if __name__ == '__main__':
    main()
