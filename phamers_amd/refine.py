"""
refine.py -- segment boundaries refined from the window grid to the base (this project's own).

``compose`` decodes windows, so every region it reports ends on the window grid.  The fitted states hold what a finer answer
needs: a profile log theta_s over the 4^k k-mers.  Around a boundary between a run of state a and a run of state b the best
change point is the prefix maximum of the per-base log ratio

    d(i) = q_a[kmer_i] - q_b[kmer_i]        q = segment.quantise(log theta): int64, units of 2^-16 nat
    P(p) = sum_{lo <= i < p} d(i)           the k-mer starting at i belongs to the left segment exactly when i < p
    p*   = arg max_{lo <= p <= hi} P(p)     ties: the smallest |p - x|, then the smallest p (x = the window boundary)

one pass over the bases, a prefix sum and an arg-max, all in exact integers on the device (refine.hip): the result does not
depend on the order of the reduction.  A k-mer with a base outside the alphabet, or running past its sequence's end, counts
0 -- the rule by which the windows were counted.  The log profiles go in untempered: tempering scales every row alike and
does not move an arg-max.

    boundaries(fasta_or_sequences, kmer_length, log_profiles, seq, lo, x, hi, left_row, right_row)     a Refined

``compose.boundary_plan`` makes the intervals from a decode; ``ComposedSequences.refine`` puts the two together.
"""
import collections

import numpy as np

from . import _lib
from .segment import QUANT_BITS, quantise

MAX_SPAN = 1 << 30

Refined = collections.namedtuple("Refined", "position gain left_evidence right_evidence support gain_nats left_evidence_nats "
                                            "right_evidence_nats")
Refined.__doc__ = """position (B,) int64: the refined change point in bases of the sequence; gain = P(position) - P(x),
left_evidence = P(position) - P(lo), right_evidence = P(position) - P(hi): (B,) int64 >= 0 in units of 2^-16 nat, and the
same as float64 nats (``*_nats``); support (B,) int64: the valid k-mers starting in [lo, hi)."""


def _refine(fasta_or_sequences, kmer_length, symbols, qtable, seq, lo, x, hi, left_row, right_row):
    """(position, evidence (B, 3), support) from the device (the tests put the statement in its place)."""
    ctx = _lib.get_context()
    if isinstance(fasta_or_sequences, str):
        fasta = _lib.Fasta(fasta_or_sequences)
        try:
            return _lib.refine_boundaries(ctx, fasta, kmer_length, symbols, qtable, seq, lo, x, hi, left_row, right_row)
        finally:
            fasta.close()
    return _lib.refine_boundaries(ctx, list(fasta_or_sequences), kmer_length, symbols, qtable, seq, lo, x, hi, left_row, right_row)


def _indices(v, name):
    a = np.asarray(v)
    if a.ndim != 1 or not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
        raise ValueError("%s must be a 1-D integer array" % name)
    a = a.astype(np.int64)
    if a.size and a.min() < 0:
        raise ValueError("%s must not be negative" % name)
    return a


def _checked(kmer_length, log_profiles, seq, lo, x, hi, left_row, right_row, symbols):
    """The arguments of ``boundaries`` checked and converted: (k, symbols, the quantised table, the six (B,) int64 arrays)."""
    from . import kmer
    symbols = kmer.DNA if symbols is None else symbols
    sym = kmer._check_symbols(symbols)
    k = int(kmer_length)
    if not 1 <= k <= _lib.MAX_K:
        raise ValueError("kmer_length must be 1 to %d, got %r" % (_lib.MAX_K, kmer_length))
    logp = np.asarray(log_profiles, dtype=np.float64)
    if logp.ndim != 2 or logp.shape[1] != 4 ** k:
        raise ValueError("log_profiles must be (n_rows, %d) for k = %d" % (4 ** k, k))
    if np.isnan(logp).any():
        raise ValueError("log_profiles must not hold NaN")
    seq, lo, x, hi = _indices(seq, "seq"), _indices(lo, "lo"), _indices(x, "x"), _indices(hi, "hi")
    left_row, right_row = _indices(left_row, "left_row"), _indices(right_row, "right_row")
    B = len(seq)
    if not all(len(a) == B for a in (lo, x, hi, left_row, right_row)):
        raise ValueError("seq, lo, x, hi, left_row and right_row must have one entry per boundary")
    if B and (max(left_row.max(), right_row.max()) >= logp.shape[0]):
        raise ValueError("a row index is outside the %d rows of log_profiles" % logp.shape[0])
    if ((lo > x) | (x > hi)).any():
        raise ValueError("every boundary needs lo <= x <= hi")
    if (hi - lo > MAX_SPAN).any():
        raise ValueError("an interval of more than 2^30 bases")
    return k, sym, quantise(logp), (seq, lo, x, hi, left_row, right_row)


def _refined(position, evidence, support):
    evidence = np.asarray(evidence, dtype=np.int64).reshape(-1, 3)
    nats = evidence.astype(np.float64) * 2.0 ** -QUANT_BITS
    return Refined(np.asarray(position, dtype=np.int64), evidence[:, 0].copy(), evidence[:, 1].copy(), evidence[:, 2].copy(),
                   np.asarray(support).astype(np.int64), nats[:, 0].copy(), nats[:, 1].copy(), nats[:, 2].copy())


def boundaries(fasta_or_sequences, kmer_length, log_profiles, seq, lo, x, hi, left_row, right_row, symbols=None):
    """Boundary b lies in sequence ``seq[b]`` (the index of a record of the FASTA file, or of a string of the list), between
    a segment whose k-mers follow row ``left_row[b]`` of ``log_profiles`` (n_rows, 4^k) and one that follows row
    ``right_row[b]``; the window grid put it at base ``x[b]``, and it is looked for in ``lo[b] .. hi[b]``
    (0 <= lo <= x <= hi <= the sequence's length, hi - lo <= 2^30).  The profiles are quantised by ``segment.quantise`` (no
    logarithm is taken here or on the device).  A ``Refined``; a boundary without evidence stays at x.  ValueError for what
    the library refuses."""
    k, sym, q, cols = _checked(kmer_length, log_profiles, seq, lo, x, hi, left_row, right_row, symbols)
    return _refined(*_refine(fasta_or_sequences, k, sym, q, *cols))


# ---- how sharp the maximum is --------------------------------------------------------------------
DEFAULT_DROP = 3.0

Confidence = collections.namedtuple("Confidence", "lower upper n_within at_lo at_hi log_z mass_at_position mass_within mean_offset "
                                                  "rms_distance sums")
Confidence.__doc__ = """Per boundary, (B,) each.  Exact: lower / upper, the smallest / largest p in [lo, hi] with
P(p) >= P(position) - drop, and n_within, how many such p there are (int64; they need not be contiguous); at_lo / at_hi (bool):
lower == lo / upper == hi -- the search interval cut the support interval short.  Float64, of the posterior
w(p) / Z, w(p) = exp(P(p) - P(position)), of one change point in [lo, hi] under a uniform prior: log_z = log Z;
mass_at_position = 1 / Z; mass_within, the mass of lower <= p <= upper; mean_offset, the posterior mean of p - position;
rms_distance, the root of the posterior mean of (p - position)^2.  sums (B, 5) float64: Z, M, S1_left, S1_right, S2 as the
device returned them."""


def drop_quantum(drop):
    """``drop`` in nats as the int64 the device compares with: floor(drop 2^16 + 0.5), and 2^62 for 2^46 nats or more (no
    prefix sum lies further than 2^62 below the maximum: every candidate is within).  ValueError for a negative or
    non-finite drop."""
    try:
        drop = float(drop)
    except (TypeError, ValueError):
        raise ValueError("drop must be a number of nats >= 0, got %r" % (drop,))
    if not np.isfinite(drop) or drop < 0:
        raise ValueError("drop must be a finite number of nats >= 0, got %r" % (drop,))
    if drop >= 2.0 ** 46:
        return 1 << 62
    return int(np.floor(drop * 2.0 ** QUANT_BITS + 0.5))


def _confidence(fasta_or_sequences, kmer_length, symbols, qtable, seq, lo, x, hi, left_row, right_row, drop_q):
    """(position, evidence (B, 3), support, interval (B, 3), sums (B, 5)) from the device (the tests put the statement in its
    place)."""
    ctx = _lib.get_context()
    if isinstance(fasta_or_sequences, str):
        fasta = _lib.Fasta(fasta_or_sequences)
        try:
            return _lib.refine_confidence(ctx, fasta, kmer_length, symbols, qtable, seq, lo, x, hi, left_row, right_row, drop_q)
        finally:
            fasta.close()
    return _lib.refine_confidence(ctx, list(fasta_or_sequences), kmer_length, symbols, qtable, seq, lo, x, hi, left_row, right_row,
                                  drop_q)


def confidence_from_sums(lo, hi, interval, sums):
    """A ``Confidence`` of the device's interval (B, 3) and sums (B, 5): the host's share -- one logarithm, three divisions
    and a root per boundary."""
    interval = np.asarray(interval, dtype=np.int64).reshape(-1, 3)
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 5)
    Z, M, left, right, S2 = (sums[:, i] for i in range(5))
    lower, upper = interval[:, 0].copy(), interval[:, 1].copy()
    return Confidence(lower, upper, interval[:, 2].copy(), lower == np.asarray(lo, dtype=np.int64), upper == np.asarray(hi, dtype=np.int64),
                      np.log(Z), 1.0 / Z, M / Z, (right - left) / Z, np.sqrt(S2 / Z), sums)


def confidence(fasta_or_sequences, kmer_length, log_profiles, seq, lo, x, hi, left_row, right_row, drop=DEFAULT_DROP, symbols=None):
    """``boundaries`` and, from a second kernel in the same call, how sharp each maximum is: ``(Refined, Confidence)``; the
    ``Refined`` is what ``boundaries`` returns, bit for bit.  ``drop`` (nats, >= 0, quantised to 2^-16 nat) sets the support
    interval: the positions whose likelihood is within a factor exp(-drop) of the best.  The default of 3 nats (relative
    likelihood e^-3, about 1/20) is a modelling choice, not a derived one: ``drop`` = 0 gives the tie class of the maximum, a
    large drop every candidate.

    The posterior assumes exactly one change point in [lo, hi] and multinomial k-mers.  Overlapping k-mers are not
    independent draws (they are over-dispersed), so the intervals and masses are optimistic."""
    k, sym, q, cols = _checked(kmer_length, log_profiles, seq, lo, x, hi, left_row, right_row, symbols)
    position, evidence, support, interval, sums = _confidence(fasta_or_sequences, k, sym, q, *cols, drop_quantum(drop))
    return _refined(position, evidence, support), confidence_from_sums(cols[1], cols[3], interval, sums)
