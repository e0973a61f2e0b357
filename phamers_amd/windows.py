"""Phage scores ALONG sequences: a score for every overlapping window of an assembled genome or a long scaffold, and the
regions the windows above a threshold merge to.

    track = score_windows("genome.fasta", positive, negative, window=5000, step=500)
    regions = call_regions(track, threshold=0.0, min_windows=2)

    python -m phamers_amd.windows -in genome.fasta -out DIR -data DATA_DIR [-w 5000 -s 500 -k 4 -m combo -t 0 -min 1]
                                  [--both_strands]

The windows are the rows of ONE device-resident batch (``kmer.count_windows``' kernel: every base goes to the device once,
whatever the overlap); normalisation and every scoring method then apply to it as to any batch of
contigs.  With ``both_strands`` the window rows are folded with their reverse complement on the device (DESIGN.md section
4.13): the track of a sequence is then the track of its reverse complement read backwards.  This is this project's own
tool: the reference scores whole contigs only.  Not here: sharding the windows over several GPUs, plots.
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
    (kmeans / combo), else None."""

    def __init__(self, record_ids, owner, start, window, step, scores, positive_centroids=None, negative_centroids=None):
        self.record_ids = list(record_ids)
        self.owner = np.asarray(owner, dtype=np.int64)
        self.start = np.asarray(start, dtype=np.int64)
        self.window, self.step = int(window), int(step)
        self.scores = np.asarray(scores, dtype=np.float64)
        self.positive_centroids, self.negative_centroids = positive_centroids, negative_centroids

    def __len__(self):
        return self.scores.shape[0]


def score_windows(fasta_file_or_sequences, positive, negative, window=5000, step=500, kmer_length=4, method='combo',
                  k_clusters=86, both_strands=False):
    """Scores every window of ``window`` bases, every ``step`` bases, of every sequence (a FASTA path or a list of strings,
    as ``kmer.count_windows``) against the normalised reference matrices ``positive`` / ``negative`` -> WindowTrack.
    A window without a single valid k-mer (a scaffold gap of N) would be a NaN query row: it is left out of the scored
    batch and its score is nan.  The model (and, for kmeans / combo, the centroids: k-means with ``k_clusters``) is built
    once per call, as ``phamer.score_contigs`` builds it.  ``both_strands``: the window rows are folded with their reverse
    complement before scoring; ``positive`` / ``negative`` are taken as given -- pass references normalised from folded
    counts (transform_kmers.fold_strands), as the command line does."""
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
            (('-m', '--method'), dict(default='combo', help='Scoring method')),
            (('-t', '--threshold'), dict(type=float, default=0.0, help='A window is a hit when its score is above this')),
            (('-min', '--min_windows'), dict(type=int, default=1, help='Fewest consecutive hits that make a region')),
            (('--both_strands',), dict(action='store_true', help='Fold windows and reference counts with their reverse '
                                                                 'complement'))):
        ap.add_argument(*flags, **kw)
    return ap


def main(argv=None):
    ap = _parser()
    args = ap.parse_args(argv)
    from . import phamer
    scorer = phamer.phamer_scorer()
    scorer.both_strands = args.both_strands      # (_load_reference folds the reference counts it reads)
    if args.data_directory:
        scorer.data_directory = args.data_directory
        scorer.find_data_files()
    scorer.positive_features_file = args.positive_features or scorer.positive_features_file
    scorer.negative_features_file = args.negative_features or scorer.negative_features_file
    if not (scorer.positive_features_file and scorer.negative_features_file):
        ap.error("give -data <dir with reference_features/> or -pf and -nf")
    scorer._load_reference()
    track = score_windows(args.fasta_file, scorer.positive_data, scorer.negative_data, window=args.window, step=args.step,
                          kmer_length=args.kmer_length, method=args.method, both_strands=args.both_strands)
    regions = call_regions(track, threshold=args.threshold, min_windows=args.min_windows)
    os.makedirs(args.output_directory, exist_ok=True)
    save_track(os.path.join(args.output_directory, "window_scores.csv"), track, args=args)
    save_regions(os.path.join(args.output_directory, "phage_regions.csv"), regions, args=args)
    return track, regions


if __name__ == '__main__':
    main()
