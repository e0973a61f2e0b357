"""
hosts.py -- likelihood-ranked reference lookup and host prediction (this project's own).

The likelihood method (likelihood.py) computes S[q, r] = sum_j c_q[j] * L[r, j] of every contig's count row against
every reference row and folds it into one number per class.  This module keeps the other half of that product: WHICH
reference rows a contig is most likely to come from.  ``learning.kneighbors`` answers that in frequency space, by
Euclidean distance, which ignores how long the contig is; the likelihood does not.

Two log tables, both built here on the host with NumPy:

    multinomial   L[r, j]      = log((x_r[j] + a) / (sum_j x_r[j] + D a))                  likelihood.log_table
    markov        L[r, 4p + b] = log((x_r[4p + b] + a) / (sum_b' x_r[4p + b'] + 4a))        markov_log_table

With the Markov table S is the log-likelihood of the contig's k-mer transitions under row r's Markov chain of order k - 1
(the initial (k-1)-mer is ignored): the composition-based host predictor of WIsH (Galiez et al. 2017, Bioinformatics 33:3113),
whose null -- per host, the mean and standard deviation of the per-k-mer log-likelihood over phage genomes -- is
``fit_null``.  The rank is by likelihood; z and p only annotate the hits (ranking by z is useless for retrieval).

    markov_log_table(counts, pseudocount)                                   (M, D) float64
    rank(query_counts, reference_counts, top, model, ...)                   Ranking
    fit_null(null_counts, reference_counts, model, pseudocount)             (mu (M,), sigma (M,))
    predict(query_counts, host_counts, null_counts, top, model='markov')    Ranking with z and p_value

The N x M product, the selection and the null's two passes run in float64 on the device (hosts.hip) from the integer rows.
What this module does not claim: the accuracy of host prediction on real phage-host pairs cannot be measured from
anything in this repository -- the reference ids are bare accessions and there is no host table.
"""
import math
from collections import namedtuple

import numpy as np

from . import _lib
from .likelihood import _count_rows, _pseudocount, log_table

MODELS = ('multinomial', 'markov')

Ranking = namedtuple("Ranking", "indices log_likelihood per_kmer z p_value")
Ranking.__doc__ = """indices (N, top) int64 into the reference rows, by (S descending, index ascending); log_likelihood
(N, top) float64, the S of the returned pairs in nats; per_kmer = S / the query's k-mers (NaN for a query without counts);
z, p_value (N, top): (per_kmer - mu[idx]) / sigma[idx] and 0.5 erfc(z / sqrt 2) under a fitted null, None without one."""


def markov_log_table(counts, pseudocount=0.5):
    """L[r, 4p + b] = log((x_r[4p + b] + a) / (sum_b' x_r[4p + b'] + 4a)) of the k-mer count rows ``counts`` (M, 4^k),
    k >= 1: float64 (M, D), NumPy on the host.  The first base of a k-mer is the most significant digit of its column
    (kmer.py), so the four k-mers that share the (k-1)-mer prefix p are columns 4p .. 4p + 3: each group is the transition
    distribution out of p of row r's chain of order k - 1.  ValueError for a D that is not a power of 4, and the rules of
    likelihood.log_table otherwise."""
    a = _pseudocount(pseudocount)
    x = _count_rows(counts, "counts").astype(np.float64)
    M, D = x.shape
    _check_width(D)
    g = x.reshape(M, D // 4, 4)
    return np.log((g + a) / (g.sum(axis=2, keepdims=True) + 4.0 * a)).reshape(M, D)


def _check_width(D):
    k = int(round(math.log(D, 4))) if D > 0 else 0
    if k < 1 or 4 ** k != D:
        raise ValueError("the Markov table needs k-mer count rows of 4^k columns (k >= 1), got %d columns" % D)


def _table(reference_counts, model, pseudocount):
    if model not in MODELS:
        raise ValueError("model must be one of %r, got %r" % (MODELS, model))
    return markov_log_table(reference_counts, pseudocount) if model == 'markov' else log_table(reference_counts, pseudocount)


def _check_rows_left(top, M, query_groups, reference_groups):
    """ValueError when ``top`` exceeds the reference rows some query has left, from the group histogram alone."""
    if query_groups is None or reference_groups is None:
        return
    rg = reference_groups[reference_groups >= 0]
    ids, per_id = np.unique(rg, return_counts=True)
    where = np.searchsorted(ids, query_groups)
    hit = (query_groups >= 0) & (where < len(ids))
    hit[hit] = ids[where[hit]] == query_groups[hit]
    left = np.full(len(query_groups), M, dtype=np.int64)
    left[hit] -= per_id[where[hit]]
    if len(left) and left.min() < top:
        q = int(np.argmin(left))
        raise ValueError("top = %d exceeds the %d reference rows query %d (group %d) has left"
                         % (top, left[q], q, query_groups[q]))


def _null(null, M):
    if null is None:
        return None
    mu, sigma = (np.asarray(v, dtype=np.float64) for v in null)
    if mu.shape != (M,) or sigma.shape != (M,):
        raise ValueError("null must be (mu, sigma) with one entry per reference row (%d), got shapes %r and %r"
                         % (M, mu.shape, sigma.shape))
    return mu, sigma


def _annotate(idx, S, totals, null):
    """The Ranking of device results: per_kmer, z and p_value are host NumPy on the returned pairs."""
    with np.errstate(invalid='ignore', divide='ignore'):
        per_kmer = S / totals.astype(np.float64)[:, None]
    if null is None:
        return Ranking(idx, S, per_kmer, None, None)
    mu, sigma = null
    with np.errstate(invalid='ignore', divide='ignore'):
        z = (per_kmer - mu[idx]) / sigma[idx]
    return Ranking(idx, S, per_kmer, z, p_value(z))


def p_value(z):
    """0.5 erfc(z / sqrt 2) (math.erfc), element by element: the upper tail of a standard normal at z; NaN for NaN."""
    z = np.asarray(z, dtype=np.float64)
    out = np.empty(z.shape, dtype=np.float64)
    flat_z, flat = z.ravel(), out.ravel()
    for i in range(flat_z.size):
        flat[i] = 0.5 * math.erfc(flat_z[i] / math.sqrt(2.0))
    return flat.reshape(z.shape)


def rank(query_counts, reference_counts, top=5, model='multinomial', pseudocount=0.5, query_groups=None,
         reference_groups=None, null=None, _batch_rows=0):
    """The ``top`` reference rows every count row of ``query_counts`` (N, D) is most likely to come from, out of the count
    rows ``reference_counts`` (M, D): a ``Ranking``.  A query's result is its first ``top`` rows in order of (S descending,
    row index ascending), S the float64 product the likelihood scorer computes; it is bit for bit the same whatever N,
    the batch split, the entry point or the run, so identical reference rows tie exactly and come in index order.
    ``model``: 'multinomial' (likelihood.log_table) or 'markov' (markov_log_table).  With group ids on both sides
    (integers; negative = none) a reference row is skipped for the queries of its own group.  ``null``: (mu, sigma) of
    fit_null for the same reference rows, model and pseudocount; z and p_value are None without it.  A query without
    counts gets rows 0..top-1 with S = 0.0, per_kmer NaN and z NaN.  ValueError for ``top`` outside
    1.._lib.HOSTS_MAX_TOP or beyond the rows a query has left (found on the host, before any launch).  ``_batch_rows``
    (queries per device batch) is for the tests, no result depends on it."""
    q = _count_rows(query_counts, "query_counts")
    L = _table(reference_counts, model, pseudocount)
    M = L.shape[0]
    if L.shape[1] != q.shape[1]:
        raise ValueError("queries and reference rows must have the same number of columns")
    if M == 0:
        raise ValueError("no reference rows")
    top = _lib.check_hosts_top(top, M)
    qg = _lib._groups(query_groups, q.shape[0], "query_groups")
    rg = _lib._groups(reference_groups, M, "reference_groups")
    _check_rows_left(top, M, qg, rg)
    null = _null(null, M)
    table = _lib.HostTable(_lib.get_context(), L, rg)
    try:
        idx, S = table.rank(q, top, qg, batch_rows=_batch_rows)
    finally:
        table.close()
    return _annotate(idx, S, q.sum(axis=1, dtype=np.uint64), null)


def fit_null(null_counts, reference_counts, model='markov', pseudocount=0.5, _batch_rows=0):
    """(mu, sigma), each (M,) float64: per reference row the mean and the sample standard deviation (ddof = 1) of
    l[p, r] = S[p, r] / n_p over the count rows ``null_counts`` (P, D), n_p the row's k-mers.  On the device, in two passes
    over the product (column sums -> mu, then the centred squares), every column accumulated in row order: no bit depends
    on ``_batch_rows``.  ValueError for P < 2 or a null row without counts."""
    x = _count_rows(null_counts, "null_counts")
    L = _table(reference_counts, model, pseudocount)
    if L.shape[1] != x.shape[1]:
        raise ValueError("null rows and reference rows must have the same number of columns")
    if L.shape[0] == 0:
        raise ValueError("no reference rows")
    if x.shape[0] < 2:
        raise ValueError("a standard deviation needs at least 2 null rows, got %d" % x.shape[0])
    if (x.sum(axis=1, dtype=np.uint64) == 0).any():
        raise ValueError("null row %d has no counts" % int(np.flatnonzero(x.sum(axis=1, dtype=np.uint64) == 0)[0]))
    table = _lib.HostTable(_lib.get_context(), L)
    try:
        return table.null_fit(x, batch_rows=_batch_rows)
    finally:
        table.close()


def predict(query_counts, host_counts, null_counts, top=5, model='markov', pseudocount=0.5, _batch_rows=0):
    """fit_null, then rank: the ``top`` most likely rows of ``host_counts`` for every query, annotated with the z-score and
    p-value of its per-k-mer log-likelihood under the host's null.  ``model`` defaults to 'markov' here -- WIsH's model and
    a proper likelihood of a sequence -- while ``rank`` defaults to 'multinomial'.  The null is fitted on EVERY row of
    ``null_counts``: when those are phage genomes, the ones that do infect a host are among them and widen that host's
    null (WIsH fits each host's null on phages known not to infect it; no such table exists here)."""
    null = fit_null(null_counts, host_counts, model, pseudocount, _batch_rows)
    return rank(query_counts, host_counts, top, model, pseudocount, null=null, _batch_rows=_batch_rows)
