"""
segment.py -- phage regions from a window track by a two-state hidden Markov chain (this project's own).

``windows.call_regions`` thresholds every window on its own: one noisy window splits a prophage, one lucky window in the
host makes a region.  Here the windows of a record are the steps of a chain with the states 0 = host and 1 = phage:

    x_t          = temper * score_t           the evidence, nats; a nan score gives x_t = 0 (no evidence: the chain carries)
    emission     e_t = (1, exp(x_t))
    transition   A = [[1 - a, a], [b, 1 - b]]   a = p_enter, b = p_leave
    start        pi = (1 - p_start, p_start)    default: the stationary a / (a + b)

and the device (segment.hip) returns, per window, the posterior P(state_t = 1 | the record's x) and the Viterbi path, and per
record the log evidence against the all-host chain and the path's score.  The two have different contracts: the path is the
plain left-to-right recurrence on exact integers (units of 2^-16 nat: ``quantise``; |x_t| is clamped to 2^15 nats there), the
posterior is float64 without cancellation, within the bound of tests/segment_ref.py.

    decode(scores, owner_or_offsets, p_enter, p_leave, p_start=None, temper=1.0)     -> Decoded
    segment_track(track, mean_region=30000, phage_fraction=0.05, temper=None)        -> Segmentation
    Segmentation.regions(min_windows=1), save_segments(filename, regions)            phage_segments.csv
    python -m phamers_amd.windows ... --segment                                      writes that file beside the other two

A score is the emission term of such a chain only when it is a log-likelihood ratio: the ``likelihood`` and ``density``
methods' scores are, the others' are not -- the decode accepts any track and cannot tell.  The configuration the chain is
meant for is non-overlapping short windows scored by the likelihood method (``-m likelihood -w 500 -s 500 --segment``).
Not here: fitting a or b, more than two states, boundaries finer than a window, several GPUs.
"""
import collections

import numpy as np

from . import _lib

QUANT_BITS = _lib.SEG_QUANT_BITS
CLAMP = 2.0 ** 15     # nats: what the integer recurrence sees of |x_t| at most

Decoded = collections.namedtuple("Decoded", "posterior state log_odds path_score path_score_q")
Decoded.__doc__ = """posterior (n,) float64, state (n,) uint8, log_odds (R,) float64, path_score (R,) float64 nats
= path_score_q (R,) int64 * 2^-16."""


def quantise(v):
    """rint(clip(v, -2^15, 2^15) * 2^16) as int64: the integer the Viterbi recurrence takes for a value in nats (ties to
    even, as rint; -0.0 gives 0).  NumPy on the host; the device quantises x_t by the same rule."""
    return np.rint(np.clip(np.asarray(v, dtype=np.float64), -CLAMP, CLAMP) * float(1 << QUANT_BITS)).astype(np.int64)


def parameters(p_enter, p_leave, p_start=None):
    """(trans (4,), init (2,), qlog_trans (4,) int64, qlog_init (2,) int64) of a = ``p_enter``, b = ``p_leave`` and
    ``p_start`` (None: the stationary a / (a + b)): the probabilities, and their logarithms -- taken here, by NumPy --
    quantised.  ValueError unless 0 < a, b, p_start < 1 and every complement 1 - p is inside (0, 1) too."""
    a, b = float(p_enter), float(p_leave)
    s = a / (a + b) if p_start is None and a + b > 0 else (np.nan if p_start is None else float(p_start))
    for name, p in (("p_enter", a), ("p_leave", b), ("p_start", s)):
        if not (0.0 < p < 1.0 and 0.0 < 1.0 - p < 1.0):
            raise ValueError("%s must lie inside (0, 1), with 1 - %s inside it too, got %r" % (name, name, p))
    trans = np.array([1.0 - a, a, b, 1.0 - b], dtype=np.float64)
    init = np.array([1.0 - s, s], dtype=np.float64)
    return trans, init, quantise(np.log(trans)), quantise(np.log(init))


def _offsets(owner_or_offsets, n):
    """uint64 (R + 1,) record offsets: an (n,) array is the non-decreasing record index of every window (as
    WindowTrack.owner) and is counted into offsets; any other length must be offsets, non-decreasing from 0 to n."""
    o = np.asarray(owner_or_offsets)
    if o.ndim != 1 or not (np.issubdtype(o.dtype, np.integer) or o.size == 0):
        raise ValueError("owner_or_offsets must be a 1-D integer array")
    o = o.astype(np.int64)
    if o.size and o.min() < 0:
        raise ValueError("owner_or_offsets must not be negative")
    is_offsets = o.size >= 1 and o[0] == 0 and o[-1] == n
    if is_offsets and o.size == n and n > 0:
        raise ValueError("an array of n = %d entries that runs from 0 to n reads both as owners and as offsets: pass the "
                         "owner of every window, np.repeat(np.arange(R), np.diff(offsets))" % n)
    if o.size == n:
        if n and (np.diff(o) < 0).any():
            raise ValueError("the owner array must be non-decreasing (windows in record order)")
        records = int(o[-1]) + 1 if n else 0
        return np.concatenate(([0], np.cumsum(np.bincount(o, minlength=records)))).astype(np.uint64)
    if not is_offsets or (np.diff(o) < 0).any():
        raise ValueError("offsets must run non-decreasing from 0 to %d" % n)
    return o.astype(np.uint64)


def evidence(scores, temper=1.0):
    """x = temper * scores as float64, nan -> 0.0; ValueError for an infinite score or a temper that is not finite and > 0."""
    t = float(temper)
    if not (np.isfinite(t) and t > 0):
        raise ValueError("temper must be finite and > 0, got %r" % (temper,))
    s = np.asarray(scores, dtype=np.float64)
    if s.ndim != 1:
        raise ValueError("scores must be 1-D")
    if np.isinf(s).any():
        raise ValueError("the scores hold an infinite value")
    with np.errstate(over='ignore'):
        x = t * s
    x[np.isnan(s)] = 0.0
    if np.isinf(x).any():
        raise ValueError("temper * scores overflows")
    return x


def decode(scores, owner_or_offsets, p_enter, p_leave, p_start=None, temper=1.0):
    """The chain of the module docstring over every record of ``scores`` (n,): ``owner_or_offsets`` is either the (n,)
    non-decreasing record index of every window (WindowTrack.owner) or the (R + 1,) offsets of the records; an array of
    exactly n entries is read as owners (ValueError when it would read as offsets too: n = R + 1 and it runs from 0 to
    n).  -> Decoded, everything computed on the device.  Only scores that are log-likelihood ratios in nats (the
    ``likelihood`` and ``density`` methods') make ``p_enter`` / ``p_leave`` mean what they say; any array is accepted."""
    trans, init, qt, qp = parameters(p_enter, p_leave, p_start)
    x = evidence(scores, temper)
    return _decode(x, _offsets(owner_or_offsets, x.shape[0]), trans, init, qt, qp)


def _decode(x, offsets, trans, init, qlog_trans, qlog_init):
    post, state, lo, ps = _lib.segment_decode(_lib.get_context(), x, offsets, trans, init, qlog_trans, qlog_init)
    return Decoded(post, state, lo, ps.astype(np.float64) * 2.0 ** -QUANT_BITS, ps)


def default_temper(window, step, kmer_length):
    """min(1, step / (window - k + 1)): overlapping windows repeat the same k-mers window / step times, and tempering the
    evidence by the inverse is the composite-likelihood correction; exactly 1 for windows that do not overlap."""
    return min(1.0, float(step) / float(max(1, int(window) - int(kmer_length) + 1)))


class Segmentation(object):
    """What ``segment_track`` returns: the track's ``record_ids``, ``owner``, ``start``, ``window``, ``step``; the evidence
    ``x`` (n,); ``posterior``, ``state`` (n,); ``log_odds``, ``path_score`` (one per record id; 0 for a record without
    windows); and the parameters ``p_enter``, ``p_leave``, ``temper``."""

    def __init__(self, track, x, decoded, p_enter, p_leave, temper):
        self.record_ids, self.owner, self.start = list(track.record_ids), track.owner, track.start
        self.window, self.step = track.window, track.step
        self.x, self.posterior, self.state = x, decoded.posterior, decoded.state
        self.log_odds, self.path_score = decoded.log_odds, decoded.path_score
        self.p_enter, self.p_leave, self.temper = p_enter, p_leave, temper

    def __len__(self):
        return self.state.shape[0]

    def regions(self, min_windows=1):
        """Per run of consecutive windows of one record with state 1: ``(record id, start of the first window, start of
        the last + window, n_windows, mean posterior, max posterior, sum of x over the run)``; runs of fewer than
        ``min_windows`` windows are dropped.  Ordered by record and start.  Host work (NumPy)."""
        n = self.state.shape[0]
        if n == 0:
            return []
        hit = self.state.astype(bool)
        joined = hit[1:] & hit[:-1] & (self.owner[1:] == self.owner[:-1])
        first = np.flatnonzero(hit & np.concatenate(([True], ~joined)))
        last = np.flatnonzero(hit & np.concatenate((~joined, [True])))
        out = []
        for a, b in zip(first, last):
            if b - a + 1 < int(min_windows):
                continue
            p = self.posterior[a:b + 1]
            out.append((self.record_ids[int(self.owner[a])], int(self.start[a]), int(self.start[b]) + self.window,
                        int(b - a + 1), float(p.mean()), float(p.max()), float(self.x[a:b + 1].sum())))
        return out


def segment_track(track, mean_region=30000, phage_fraction=0.05, temper=None, kmer_length=4):
    """Decodes a ``windows.WindowTrack``: p_leave = step / ``mean_region`` (the mean length of a phage region in bases;
    must be < 1), p_enter = p_leave * f / (1 - f) with f = ``phage_fraction`` (the stationary share of phage windows), the
    start distribution stationary.  ``temper=None``: ``default_temper(window, step, kmer_length)``.  The two defaults are
    modelling choices -- a prophage of tens of kb, a few per cent of a bacterial genome -- not measurements.  The track may
    come from any method, but only ``likelihood`` and ``density`` scores are log-likelihood ratios.  -> Segmentation."""
    f = float(phage_fraction)
    if not 0.0 < f < 1.0:
        raise ValueError("phage_fraction must lie inside (0, 1), got %r" % (phage_fraction,))
    if not float(mean_region) > 0:
        raise ValueError("mean_region must be > 0, got %r" % (mean_region,))
    b = float(track.step) / float(mean_region)
    if not b < 1.0:
        raise ValueError("mean_region = %r must exceed the step of %d bases" % (mean_region, track.step))
    a = b * f / (1.0 - f)
    t = default_temper(track.window, track.step, kmer_length) if temper is None else float(temper)
    trans, init, qt, qp = parameters(a, b)
    x = evidence(track.scores, t)
    records = len(track.record_ids)
    off = np.concatenate(([0], np.cumsum(np.bincount(track.owner, minlength=records)))).astype(np.uint64) \
        if len(track.owner) else np.zeros(records + 1, dtype=np.uint64)
    return Segmentation(track, x, _decode(x, off, trans, init, qt, qp), a, b, t)


COLUMNS = "record_id,start,end,n_windows,mean_posterior,max_posterior,sum_evidence"


def save_segments(filename, regions, args=None):
    """``phage_segments.csv``, in the style of ``windows.save_regions``: the '# ' comment header (the argument summary when
    ``args`` is given, then the column names), then one line per region of ``Segmentation.regions``."""
    from . import fileIO, windows
    header = "PhaMers phage segment file"
    if args is not None:
        header = fileIO.generate_summary(args, header=header).rstrip('\n')
    windows._write_csv(filename, header, COLUMNS, ["%s,%d,%d,%d,%r,%r,%r\n" % tuple(r) for r in regions])


def read_segments(filename):
    """The regions of a file ``save_segments`` wrote, as ``Segmentation.regions`` returns them."""
    out = []
    with open(filename, 'r') as f:
        for line in f:
            if line.startswith('#') or not line.strip():
                continue
            rid, s, e, n, mean, mx, sx = line.rstrip('\n').rsplit(',', 6)
            out.append((rid, int(s), int(e), int(n), float(mean), float(mx), float(sx)))
    return out
