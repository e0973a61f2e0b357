"""Phage scores ALONG sequences: a score for every overlapping window of an assembled genome or a long scaffold, and the
regions the windows above a threshold merge to.

    track = score_windows("genome.fasta", positive, negative, window=5000, step=500)
    regions = call_regions(track, threshold=0.0, min_windows=2)

    python -m phamers_amd.windows -in genome.fasta -out DIR -data DATA_DIR [-w 5000 -s 500 -k 4 -m combo -t 0 -min 1]
                                  [--both_strands] [--pseudocount A]
                                  [--segment [--mean_region N --phage_fraction F --temper T]
                                             [--fit [--fit_iterations N --fit_tolerance T --fit_start stationary|free]]]

The windows are the rows of ONE device-resident batch (``kmer.count_windows``' kernel: every base goes to the device once,
whatever the overlap); normalisation and every scoring method then apply to it as to any batch of
contigs.  With ``both_strands`` the window rows are folded with their reverse complement on the device (DESIGN.md section
4.13): the track of a sequence is then the track of its reverse complement read backwards.  This is this project's own
tool: the reference scores whole contigs only.  ``method='likelihood'`` scores the window's integer count rows against
the reference COUNT rows (likelihood.py): windows are the short sequences that method was built
for.  ``--segment`` decodes the track with a two-state hidden Markov chain on the device (segment.py, DESIGN.md section
4.22) and writes phage_segments.csv beside the other two files; with ``--fit`` the chain's transition probabilities are first
fitted to the track itself (Baum-Welch; --mean_region and --phage_fraction are the starting point),
the decode uses the fitted chain, and segment_fit.csv holds the fit's trace.  Not here: sharding the windows over several GPUs, plots.
"""
import argparse
import os

import numpy as np

from . import fileIO
from . import kmer


class WindowTrack(object):
    """The result of ``score_windows``: ``record_ids`` (one per input record), and per window, in row order, ``owner``
    (index into record_ids), ``start`` (0-based), ``scores`` (float64; nan for a window without a single valid k-mer);
    ``window`` and ``step`` as given.  ``positive_centroids`` / ``negative_centroids``: the centroids the call fitted
    (kmeans / combo), else None.  ``l_pos`` / ``l_neg``: the two class terms of the likelihood method (float64, nan where
    the score is nan; ``scores == l_pos - l_neg`` bit for bit), None for every other method."""

    def __init__(self, record_ids, owner, start, window, step, scores, positive_centroids=None, negative_centroids=None,
                 l_pos=None, l_neg=None):
        self.record_ids = list(record_ids)
        self.owner = np.asarray(owner, dtype=np.int64)
        self.start = np.asarray(start, dtype=np.int64)
        self.window, self.step = int(window), int(step)
        self.scores = np.asarray(scores, dtype=np.float64)
        self.positive_centroids, self.negative_centroids = positive_centroids, negative_centroids
        self.l_pos = None if l_pos is None else np.asarray(l_pos, dtype=np.float64)
        self.l_neg = None if l_neg is None else np.asarray(l_neg, dtype=np.float64)

    def __len__(self):
        return self.scores.shape[0]


def score_windows(fasta_file_or_sequences, positive, negative, window=5000, step=500, kmer_length=4, method='combo',
                  k_clusters=86, both_strands=False, pseudocount=0.5):
    """Scores every window of ``window`` bases, every ``step`` bases, of every sequence (a FASTA path or a list of strings,
    as ``kmer.count_windows``) against the normalised reference matrices ``positive`` / ``negative`` -> WindowTrack.
    A window without a single valid k-mer (a scaffold gap of N) would be a NaN query row: it is left out of the scored
    batch and its score is nan.  The model (and, for kmeans / combo, the centroids: k-means with ``k_clusters``) is built
    once per call, as ``phamer.score_contigs`` builds it.  ``both_strands``: the window rows are folded with their reverse
    complement before scoring; ``positive`` / ``negative`` are taken as given -- pass references normalised from folded
    counts (transform_kmers.fold_strands), as the command line does.  ``method='likelihood'``: ``positive`` /
    ``negative`` are the reference COUNT rows (ValueError for frequencies), smoothed with ``pseudocount``; the window rows
    are scored in place by ``Batch.likelihood`` -- no k-means, no model -- and the track carries ``l_pos`` / ``l_neg``."""
    if method == 'likelihood':
        return _score_windows_likelihood(fasta_file_or_sequences, positive, negative, window, step, kmer_length,
                                         both_strands, pseudocount)
    from . import phamer
    record_ids, lengths, batch = kmer._windows_batch(fasta_file_or_sequences, kmer_length, window, step)
    owner, start = kmer.window_plan(lengths, window, step)
    scores = np.full(owner.shape[0], np.nan, dtype=np.float64)
    if batch is None:
        return WindowTrack(record_ids, owner, start, window, step, scores)
    scorer = phamer.phamer_scorer()
    try:
        good = np.flatnonzero(batch.row_sums() > 0)
        if good.shape[0] < batch.n:
            chosen = batch.select(good)
            batch.close()
            batch = chosen
        if batch.n:
            if both_strands:
                batch.fold_strands()
            scorer.scoring_method, scorer.kmer_length, scorer.k_clusters = method, int(kmer_length), int(k_clusters)
            scorer.positive_data, scorer.negative_data = positive, negative
            scorer._batch = batch
            scores[good] = scorer.score_points()
    finally:
        scorer._batch = None
        batch.close()
    return WindowTrack(record_ids, owner, start, window, step, scores, scorer.positive_centroids, scorer.negative_centroids)


def _score_windows_likelihood(fasta_file_or_sequences, positive, negative, window, step, kmer_length, both_strands,
                              pseudocount):
    from . import _lib, likelihood
    log_pos = likelihood.log_table(likelihood._count_rows(positive, "positive"), pseudocount)
    log_neg = likelihood.log_table(likelihood._count_rows(negative, "negative"), pseudocount)
    if log_pos.shape[0] == 0 or log_neg.shape[0] == 0:
        raise ValueError("a class without reference rows")
    if log_pos.shape[1] != 4 ** int(kmer_length) or log_neg.shape[1] != 4 ** int(kmer_length):
        raise ValueError("the reference count rows must have 4^%d columns" % int(kmer_length))
    record_ids, lengths, batch = kmer._windows_batch(fasta_file_or_sequences, kmer_length, window, step)
    owner, start = kmer.window_plan(lengths, window, step)
    scores, l_pos, l_neg = (np.full(owner.shape[0], np.nan, dtype=np.float64) for _ in range(3))
    if batch is None:
        return WindowTrack(record_ids, owner, start, window, step, scores, l_pos=l_pos, l_neg=l_neg)
    table = None
    try:
        good = np.flatnonzero(batch.row_sums() > 0)    # (an all-zero row would score 0.0, not nan)
        if good.shape[0] < batch.n:
            chosen = batch.select(good)
            batch.close()
            batch = chosen
        if batch.n:
            if both_strands:
                batch.fold_strands()
            table = _lib.LikelihoodTable(_lib.get_context(), log_pos, log_neg)
            details = {}
            scores[good] = batch.likelihood(table, details)
            l_pos[good], l_neg[good] = details["l_pos"], details["l_neg"]
    finally:
        if table is not None:
            table.close()
        batch.close()
    return WindowTrack(record_ids, owner, start, window, step, scores, l_pos=l_pos, l_neg=l_neg)


def call_regions(track, threshold=0.0, min_windows=1):
    """The runs of consecutive windows of one record with ``score > threshold`` (a nan window ends a run), each merged to
    ``(record id, start of the first window, start of the last + window, n_windows, mean score, max score)``; runs of
    fewer than ``min_windows`` windows are dropped.  Ordered by record and start.  Host work (NumPy)."""
    scores, owner = track.scores, track.owner
    n = scores.shape[0]
    if n == 0:
        return []
    hit = np.zeros(n, dtype=bool)
    np.greater(scores, threshold, out=hit, where=~np.isnan(scores))
    joined = hit[1:] & hit[:-1] & (owner[1:] == owner[:-1])       # window i + 1 continues the run of window i
    first = np.flatnonzero(hit & np.concatenate(([True], ~joined)))
    last = np.flatnonzero(hit & np.concatenate((~joined, [True])))
    regions = []
    for a, b in zip(first, last):
        if b - a + 1 < int(min_windows):
            continue
        s = scores[a:b + 1]
        regions.append((track.record_ids[int(owner[a])], int(track.start[a]), int(track.start[b]) + track.window,
                        int(b - a + 1), float(s.mean()), float(s.max())))
    return regions


def _write_csv(filename, header, columns, rows):
    with open(filename, 'wb') as f:
        f.write(fileIO._comment_block(header + '\n' + columns))
        f.write(''.join(rows).encode('latin-1'))


def save_track(filename, track, args=None):
    """``window_scores.csv``: a '# ' comment header (the argument summary when ``args`` is given, then the column names),
    then one 'record id,start,end,score' line per window; scores as ``repr(float)`` prints them ('nan' for a window that
    could not be scored)."""
    header = "PhaMers window score file"
    if args is not None:
        header = fileIO.generate_summary(args, header=header).rstrip('\n')
    end = track.start + track.window
    _write_csv(filename, header, "record_id,start,end,score",
               ["%s,%d,%d,%r\n" % (track.record_ids[int(o)], s, e, float(v))
                for o, s, e, v in zip(track.owner, track.start, end, track.scores)])


def read_track(filename):
    """(record ids, start, end, scores) of a file ``save_track`` wrote, one entry per window."""
    ids, start, end, scores = [], [], [], []
    with open(filename, 'r') as f:
        for line in f:
            if line.startswith('#') or not line.strip():
                continue
            rid, s, e, v = line.rstrip('\n').rsplit(',', 3)
            ids.append(rid)
            start.append(int(s))
            end.append(int(e))
            scores.append(float(v))
    return ids, np.array(start, dtype=np.int64), np.array(end, dtype=np.int64), np.array(scores, dtype=np.float64)


def save_regions(filename, regions, args=None):
    """``phage_regions.csv``: the same kind of header, then one 'record id,start,end,n_windows,mean_score,max_score' line
    per region of ``call_regions``."""
    header = "PhaMers phage region file"
    if args is not None:
        header = fileIO.generate_summary(args, header=header).rstrip('\n')
    _write_csv(filename, header, "record_id,start,end,n_windows,mean_score,max_score",
               ["%s,%d,%d,%d,%r,%r\n" % tuple(r) for r in regions])


def _parser():
    ap = argparse.ArgumentParser(description='Scores overlapping windows along sequences and calls phage regions',
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    for flags, kw in (
            (('-in', '--fasta_file'), dict(required=True, help='FASTA file of the sequences to scan')),
            (('-out', '--output_directory'), dict(required=True, help='Directory for window_scores.csv and phage_regions.csv')),
            (('-data', '--data_directory'), dict(help='Directory containing reference_features/')),
            (('-pf', '--positive_features'), dict(help='Positive reference features CSV')),
            (('-nf', '--negative_features'), dict(help='Negative reference features CSV')),
            (('-w', '--window'), dict(type=int, default=5000, help='Window length in bases')),
            (('-s', '--step'), dict(type=int, default=500, help='Bases between window starts')),
            (('-k', '--kmer_length'), dict(type=int, default=4, help='k-mer length')),
            (('-m', '--method'), dict(default='combo', help='Scoring method; likelihood scores the window counts against '
                                                            'the reference counts')),
            (('-t', '--threshold'), dict(type=float, default=0.0, help='A window is a hit when its score is above this')),
            (('-min', '--min_windows'), dict(type=int, default=1, help='Fewest consecutive hits that make a region')),
            (('--both_strands',), dict(action='store_true', help='Fold windows and reference counts with their reverse '
                                                                 'complement')),
            (('--pseudocount',), dict(type=float, default=0.5, help='Pseudocount of the reference profiles (-m likelihood)')),
            (('--segment',), dict(action='store_true',
                                  help='Also decode the track with a two-state hidden Markov chain and write '
                                       'phage_segments.csv; meant for -m likelihood -w 500 -s 500 --segment')),
            (('--mean_region',), dict(type=float, default=30000, help='--segment: mean length of a phage region in bases')),
            (('--phage_fraction',), dict(type=float, default=0.05, help='--segment: stationary share of phage windows')),
            (('--temper',), dict(type=float, default=None,
                                 help='--segment: factor on the scores (default: min(1, step / (window - k + 1)))')),
            (('--fit',), dict(action='store_true',
                              help='--segment: fit the transition probabilities to the track (Baum-Welch) from --mean_region '
                                   'and --phage_fraction, decode with the fitted chain and write segment_fit.csv')),
            (('--fit_iterations',), dict(type=int, default=200, help='--fit: most M-steps')),
            (('--fit_tolerance',), dict(type=float, default=1e-8, help='--fit: relative gain of log evidence that ends the fit')),
            (('--fit_start',), dict(choices=('stationary', 'free'), default='stationary',
                                    help='--fit: the start distribution, tied to the stationary one or fitted freely'))):
        ap.add_argument(*flags, **kw)
    return ap


_SEGMENT_FLAGS = ("segment", "mean_region", "phage_fraction", "temper")
_FIT_FLAGS = ("fit", "fit_iterations", "fit_tolerance", "fit_start")


def _without(args, names):
    """``args`` without the attributes ``names`` (for the files' argument summary)."""
    return argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in names})


def main(argv=None):
    ap = _parser()
    args = ap.parse_args(argv)
    if args.fit and not args.segment:
        ap.error("--fit fits the chain of --segment: give both")
    from . import phamer
    scorer = phamer.phamer_scorer()
    scorer.both_strands = args.both_strands      # (_load_reference folds the reference counts it reads)
    scorer.keep_reference_counts = args.method == 'likelihood'
    if args.data_directory:
        scorer.data_directory = args.data_directory
        scorer.find_data_files()
    scorer.positive_features_file = args.positive_features or scorer.positive_features_file
    scorer.negative_features_file = args.negative_features or scorer.negative_features_file
    if not (scorer.positive_features_file and scorer.negative_features_file):
        ap.error("give -data <dir with reference_features/> or -pf and -nf")
    scorer._load_reference()
    likelihood = args.method == 'likelihood'
    track = score_windows(args.fasta_file, scorer.positive_counts if likelihood else scorer.positive_data,
                          scorer.negative_counts if likelihood else scorer.negative_data, window=args.window, step=args.step,
                          kmer_length=args.kmer_length, method=args.method, both_strands=args.both_strands,
                          pseudocount=args.pseudocount)
    regions = call_regions(track, threshold=args.threshold, min_windows=args.min_windows)
    os.makedirs(args.output_directory, exist_ok=True)
    # the two existing files are byte for byte what they were: --segment adds nothing to them, and they name the
    # pseudocount only where it is used; --fit adds nothing to phage_segments.csv unless it is given
    shown = _without(args, _SEGMENT_FLAGS + _FIT_FLAGS + (() if likelihood else ("pseudocount",)))
    save_track(os.path.join(args.output_directory, "window_scores.csv"), track, args=shown)
    save_regions(os.path.join(args.output_directory, "phage_regions.csv"), regions, args=shown)
    if args.segment:
        from . import segment
        fit_options = dict(p_start=args.fit_start, max_iter=args.fit_iterations, tol=args.fit_tolerance) if args.fit else {}
        seg = segment.segment_track(track, mean_region=args.mean_region, phage_fraction=args.phage_fraction,
                                    temper=args.temper, kmer_length=args.kmer_length, fit=args.fit, **fit_options)
        stamped = args if args.fit else _without(args, _FIT_FLAGS)
        segment.save_segments(os.path.join(args.output_directory, "phage_segments.csv"), seg.regions(args.min_windows),
                              args=stamped)
        if args.fit:
            segment.save_fit(os.path.join(args.output_directory, "segment_fit.csv"), seg.fit, args=args)
    return track, regions


if __name__ == '__main__':
    main()
