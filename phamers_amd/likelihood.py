"""
likelihood.py -- length-aware multinomial likelihood scoring (this project's own method).

Every other scoring method sees a contig as its normalised k-mer frequencies; this one scores the integer count row ``c``
itself, by the log-likelihood ratio of two mixtures of multinomials with one component per reference row:

    p_r[j]   = (x_r[j] + a) / (sum_j x_r[j] + D*a)       reference row r, pseudocount a (default 0.5)
    S[q, r]  = sum_j c_q[j] * log p_r[j]                 (the multinomial coefficient cancels in the ratio)
    l_C(q)   = logsumexp_{r in class C, not excluded for q} S[q, r]  -  log n_eff(q, C)
    score(q) = l_+(q) - l_-(q)                           nats; >= 0 reads as phage

S[q, r] = -n (H(q) + KL(q || p_r)) with n the row's k-mers: a kernel density whose width shrinks by itself with the length
of the contig.  There is no bandwidth, no k, no fit.  The log table is built here, on the host (``log_table``), and
uploaded once per call; the N x M product and the log-sum-exp run in float64 on the device (likelihood.hip), from the
integer rows.  A row is excluded for a query when both carry the same group id >= 0 (cross-validation: the fold).

    log_table(counts, pseudocount)                                        (M, D) float64
    log_likelihood(query_counts, reference_counts, ...)                   (N,)   one class, l_C
    score(query_counts, positive_counts, negative_counts, ...)            (N,)   l_+ - l_-
    cross_validate(positive_counts, negative_counts, folds, seed, ...)    every row scored with its own fold excluded
    python -m phamers_amd.likelihood -pf FILE -nf FILE -N FOLDS ...       length,auc,accuracy table

``--lengths`` simulates short contigs: each held-out row is replaced by a multinomial draw of n k-mers from its own
frequencies (seeded, on the host).  The simulation ignores that consecutive k-mers of a real contig overlap in k - 1
bases and so are not independent draws, and that a real fragment comes from one place of its genome, not from the
genome's average composition: real short contigs are noisier than these.
"""
import numpy as np

from . import _lib


def _count_rows(counts, what):
    """uint32 C-contiguous (n, D) count rows of ``counts``, or the ValueError of this module's argument rules."""
    c = np.asarray(counts)
    if c.ndim == 1:
        c = c[None, :]
    if c.ndim != 2 or c.shape[1] == 0:
        raise ValueError("%s must be a 2-D matrix of k-mer counts, got shape %r" % (what, np.shape(counts)))
    if c.dtype == np.bool_ or not (np.issubdtype(c.dtype, np.integer) or np.issubdtype(c.dtype, np.floating)):
        raise ValueError("%s must hold k-mer counts (integers), got dtype %s" % (what, c.dtype))
    if np.issubdtype(c.dtype, np.floating) and not (np.isfinite(c).all() and (c == np.floor(c)).all()):
        raise ValueError("%s must hold k-mer counts, not frequencies: the likelihood method needs the integer count rows "
                         "(fileIO.read_feature_file(..., normalize=False))" % what)
    if c.size and (c.min() < 0 or c.max() >= 2 ** 32):
        raise ValueError("%s must hold counts in [0, 2^32)" % what)
    return np.ascontiguousarray(c, dtype=np.uint32)


def _pseudocount(pseudocount):
    a = float(pseudocount)
    if not (np.isfinite(a) and a > 0):
        raise ValueError("pseudocount must be finite and > 0 (a zero profile entry has no logarithm), got %r" % (pseudocount,))
    return a


def log_table(counts, pseudocount=0.5):
    """log p_r[j] = log((x_r[j] + a) / (sum_j x_r[j] + D*a)) of the count rows ``counts`` (M, D): float64 (M, D), NumPy on
    the host.  ValueError for a pseudocount that is not finite and > 0, and for rows that are not counts."""
    a = _pseudocount(pseudocount)
    x = _count_rows(counts, "counts").astype(np.float64)
    return np.log((x + a) / (x.sum(axis=1, keepdims=True) + x.shape[1] * a))


def _run(query_counts, positive_counts, negative_counts, pseudocount, query_groups, positive_groups, negative_groups,
         batch_rows=0, details=None):
    q = _count_rows(query_counts, "query_counts")
    log_pos = log_table(positive_counts, pseudocount)
    log_neg = None if negative_counts is None else log_table(negative_counts, pseudocount)
    if log_pos.shape[1] != q.shape[1] or (log_neg is not None and log_neg.shape[1] != q.shape[1]):
        raise ValueError("queries and reference rows must have the same number of columns")
    if log_pos.shape[0] == 0 or (log_neg is not None and log_neg.shape[0] == 0):
        raise ValueError("a class without reference rows")
    table = _lib.LikelihoodTable(_lib.get_context(), log_pos, log_neg, positive_groups, negative_groups)
    try:
        return table.score(q, query_groups, batch_rows=batch_rows, details=details)
    finally:
        table.close()


def log_likelihood(query_counts, reference_counts, pseudocount=0.5, query_groups=None, reference_groups=None):
    """l_C(q) of every count row of ``query_counts`` (N, D) under the mixture of the rows ``reference_counts`` (M, D):
    (N,) float64, the one-class counterpart of learning.log_density.  With group ids on both sides (integers; negative =
    none) a reference row is left out for the queries of its own group; ValueError when that leaves a query no row."""
    return _run(query_counts, reference_counts, None, pseudocount, query_groups, reference_groups, None)


def score(query_counts, positive_counts, negative_counts, pseudocount=0.5, per_kmer=False, _batch_rows=0, _details=None):
    """l_+(q) - l_-(q) in nats for every count row of ``query_counts`` (N, D): (N,) float64.  ``per_kmer``: divided by the
    row's total (on the host), which ranks contigs of mixed lengths better and full-length ones slightly worse.  A row
    without counts scores exactly 0.0 (nan with ``per_kmer``).  ``_batch_rows`` (queries per device batch) is for the
    tests, no result depends on it; ``_details``: a dict that receives 'l_pos' and 'l_neg'."""
    s = _run(query_counts, positive_counts, negative_counts, pseudocount, None, None, None, _batch_rows, _details)
    return _per_kmer(s, query_counts) if per_kmer else s


def _per_kmer(scores, counts):
    totals = _count_rows(counts, "counts").sum(axis=1, dtype=np.uint64).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return scores / totals


def thin(counts, n, rng):
    """Every row replaced by a multinomial draw of ``n`` k-mers from its own frequencies (``rng``: a
    np.random.RandomState); see the module docstring for what this simulation ignores."""
    c = _count_rows(counts, "counts").astype(np.float64)
    p = c / c.sum(axis=1, keepdims=True)
    return np.stack([rng.multinomial(int(n), row) for row in p]).astype(np.uint32) if len(p) else c.astype(np.uint32)


def cross_validate(positive_counts, negative_counts, folds, seed=None, pseudocount=0.5, per_kmer=False, _queries=None,
                   _plan=None):
    """Every reference row scored with the rows of its own fold left out of both classes: the fold plan is
    cross_validate.FoldPlan's (the validator's split for the same ``folds`` and ``seed``), the fold is the group id on
    both sides, and the whole run is one device call.  ``folds='loo'``: every row is its own group.  Returns
    (positive_scores, negative_scores).  ``_queries``: (positive, negative) count rows scored in place of the reference
    rows, one for one (the command line's thinned rows); ``_plan``: a FoldPlan already drawn (the validator's)."""
    pos, neg = _count_rows(positive_counts, "positive_counts"), _count_rows(negative_counts, "negative_counts")
    if folds == 'loo':
        g_pos, g_neg = np.arange(len(pos)), len(pos) + np.arange(len(neg))
    else:
        from .cross_validate import FoldPlan
        plan = _plan or FoldPlan(len(pos), len(neg), folds, seed)
        g_pos, g_neg = plan.positive, plan.negative
    q_pos, q_neg = (pos, neg) if _queries is None else (_count_rows(_queries[0], "queries"), _count_rows(_queries[1], "queries"))
    if len(q_pos) != len(pos) or len(q_neg) != len(neg):
        raise ValueError("one query row per reference row")
    q = np.vstack((q_pos, q_neg))
    s = _run(q, pos, neg, pseudocount, np.concatenate((g_pos, g_neg)), g_pos, g_neg)
    if per_kmer:
        s = _per_kmer(s, q)
    return s[:len(pos)], s[len(pos):]


def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="Cross-validated multinomial likelihood scoring of two count files",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument('-pf', '--positive_features_file', required=True, help="Positive features (count) file")
    ap.add_argument('-nf', '--negative_features_file', required=True, help="Negative features (count) file")
    ap.add_argument('-N', '--N_fold', required=True, help="Folds of the cross validation, or 'loo'")
    ap.add_argument('--seed', type=int, default=None, help="Seed of the fold assignment and of the thinning draws")
    ap.add_argument('--pseudocount', type=float, default=0.5, help="Pseudocount of the reference profiles")
    ap.add_argument('--per_kmer', action='store_true', help="Divide every score by its row's k-mers")
    ap.add_argument('--lengths', type=int, nargs='+', default=[], metavar='n',
                    help="Also score the held-out rows thinned to n k-mers each (a multinomial draw)")
    ap.add_argument('-out', '--output_file', default=None, help="CSV to write (default: standard output)")
    return ap


def evaluate(positive_scores, negative_scores):
    """(ROC area, accuracy at threshold 0) of a scoring, both on the device (learning.predictor_performance, truth_counts)."""
    from . import learning
    tp, fp, fn, tn = learning.truth_counts(positive_scores, negative_scores, 0)
    return learning.predictor_performance(positive_scores, negative_scores)[2], float(tp + tn) / (tp + fp + fn + tn)


def main(argv=None):
    """``length,auc,accuracy`` lines: ``full`` for the rows as they are, then one line per ``--lengths`` value."""
    import sys
    from . import fileIO
    ap = _parser()
    args = ap.parse_args(argv)
    folds = 'loo' if args.N_fold == 'loo' else int(args.N_fold)
    _pseudocount(args.pseudocount)
    _, pos = fileIO.read_feature_file(args.positive_features_file)
    _, neg = fileIO.read_feature_file(args.negative_features_file)
    lines = ["length,auc,accuracy"]
    rng = np.random.RandomState(args.seed)
    for n in [None] + list(args.lengths):
        queries = None if n is None else (thin(pos, n, rng), thin(neg, n, rng))
        ps, ns = cross_validate(pos, neg, folds, args.seed, args.pseudocount, args.per_kmer, _queries=queries)
        lines.append("%s,%r,%r" % (("full" if n is None else n,) + tuple(float(v) for v in evaluate(ps, ns))))
    text = "\n".join(lines) + "\n"
    if args.output_file:
        with open(args.output_file, 'w') as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
