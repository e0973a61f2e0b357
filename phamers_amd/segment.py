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

The two transition probabilities and the start need not be guessed: ``fit`` chooses them by maximum likelihood from the
tracks themselves (Baum-Welch).  With e_t = (1, exp x_t) the sum of the records' log_odds is the
log-likelihood of the tracks under the chain, up to a term no parameter enters; the E-step -- every window's pairwise
posteriors, summed -- and the sums over the records run on the device, on a track that goes up once.

    expected_counts(scores, owner_or_offsets, p_enter, p_leave, p_start=None, temper=1.0)   -> Expected (one E-step)
    fit(scores, owner_or_offsets, p_enter, p_leave, p_start='stationary', ...)               -> Fit
    fit_track(track, mean_region=30000, phage_fraction=0.05, temper=None, ...)               -> Fit
    segment_track(track, ..., fit=True)                                                      fits, then decodes
    python -m phamers_amd.windows ... --segment --fit                                        the same; writes segment_fit.csv

``temper`` is NOT fitted, and cannot be: it is a factor on the evidence, not a parameter of the chain, and the evidence
sum grows without bound in it.

A score is the emission term of such a chain only when it is a log-likelihood ratio: the ``likelihood`` and ``density``
methods' scores are, the others' are not -- the decode accepts any track and cannot tell.  The configuration the chain is
meant for is non-overlapping short windows scored by the likelihood method (``-m likelihood -w 500 -s 500 --segment``).
Not here: more than two states, one fit per record, boundaries finer than a window, several GPUs.
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


Expected = collections.namedtuple("Expected", "transitions start log_odds totals log_evidence")
Expected.__doc__ = """transitions (R, 4) = xi(0->0), xi(0->1), xi(1->0), xi(1->1) per record, start (R, 2) = gamma_0(0),
gamma_0(1), log_odds (R,), totals (6,) = the sums of the six columns over the records, log_evidence = the sum of log_odds."""


def expected_counts(scores, owner_or_offsets, p_enter, p_leave, p_start=None, temper=1.0):
    """One E-step of the chain of the module docstring, arguments as ``decode``: per record the expected number of each of
    the four transitions, xi(i->j) = sum_{t >= 1} P(s_{t-1} = i, s_t = j | x), and the posterior of its first window's
    state; their sums over the records by a tree fixed by the record index (so the totals are a function of the per-record
    values alone), and the log evidence.  ``log_odds`` is bit for bit ``decode``'s.  -> Expected, computed on the device
    within the bound of tests/segment_fit_ref.py."""
    trans, init, _, _ = parameters(p_enter, p_leave, p_start)
    x = evidence(scores, temper)
    counts, totals, lo, ev = _lib.segment_expect(_lib.get_context(), x, _offsets(owner_or_offsets, x.shape[0]), trans, init)
    return Expected(counts[:, :4].copy(), counts[:, 4:].copy(), lo, totals, ev)


P_MIN, P_MAX = 1e-12, 1.0 - 1e-12     # what a fitted probability is clamped to
TRACE_COLUMNS = ("p_enter", "p_leave", "p_start", "n00", "n01", "n10", "n11", "g0", "g1", "log_evidence")
_START_MODES = {"stationary": _lib.SEG_START_STATIONARY, "free": _lib.SEG_START_FREE}


class Fit(object):
    """What ``fit`` returns: ``p_enter``, ``p_leave``, ``p_start`` (the fitted values); ``trace`` (n_iter + 1, 10), one row
    per iterate with the columns TRACE_COLUMNS -- the parameters, the six expected-count totals and the log evidence AT
    those parameters, the last row being the returned values'; ``log_evidence`` (the last row's); ``n_iter``; ``converged``,
    ``clamped`` (some M-step left [1e-12, 1 - 1e-12] and was put back), ``no_transitions`` (some M-step found a row of the
    transition matrix without expected counts and kept its parameter); ``temper``.  ``fit_track`` adds ``mean_region`` =
    step / p_leave and ``phage_fraction`` = a / (a + b), per trace row too (``mean_regions``, ``phage_fractions``)."""

    def __init__(self, trace, n_iter, status, fitted, temper, step=None):
        self.p_enter, self.p_leave, self.p_start = (float(v) for v in fitted)
        self.trace, self.n_iter, self.temper = trace, n_iter, temper
        self.log_evidence = float(trace[-1, 9])
        self.converged = bool(status & _lib.SEG_FIT_CONVERGED)
        self.clamped = bool(status & _lib.SEG_FIT_CLAMPED)
        self.no_transitions = bool(status & _lib.SEG_FIT_NO_TRANSITIONS)
        self.step = step
        if step is not None:
            self.mean_regions = float(step) / trace[:, 1]
            self.phage_fractions = trace[:, 0] / (trace[:, 0] + trace[:, 1])
            self.mean_region = float(step) / self.p_leave
            self.phage_fraction = self.p_enter / (self.p_enter + self.p_leave)


def _fit(x, offsets, a, b, p_start, prior_counts, max_iter, tol, temper, step=None):
    if isinstance(p_start, str):
        if p_start not in _START_MODES:
            raise ValueError("p_start must be 'stationary', 'free' or a probability, got %r" % (p_start,))
        mode, s = _START_MODES[p_start], None
    else:
        mode, s = _lib.SEG_START_FIXED, float(p_start)
    _, init, _, _ = parameters(a, b, s)
    prior = np.asarray(prior_counts, dtype=np.float64)
    if prior.shape != (4,) or not (np.isfinite(prior).all() and (prior >= 0).all()):
        raise ValueError("prior_counts must be four finite pseudo-counts >= 0 (c00, c01, c10, c11), got %r" % (prior_counts,))
    if int(max_iter) != max_iter or not 0 <= int(max_iter) <= _lib.SEG_FIT_MAX_ITER:
        raise ValueError("max_iter must be an integer in [0, %d], got %r" % (_lib.SEG_FIT_MAX_ITER, max_iter))
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError("tol must be finite and >= 0, got %r" % (tol,))
    trace, n_iter, status, fitted = _lib.segment_fit(_lib.get_context(), x, offsets, [float(a), float(b), init[1]], mode, prior,
                                                     int(max_iter), float(tol))
    return Fit(trace, n_iter, status, fitted, temper, step)


def fit(scores, owner_or_offsets, p_enter, p_leave, p_start='stationary', temper=1.0, prior_counts=(0, 0, 0, 0), max_iter=200,
        tol=1e-8):
    """Maximum-likelihood ``p_enter``, ``p_leave`` (and start) of the chain for these tracks by Baum-Welch, started at the
    values given; the records share one chain.  The scores go to the device once; an iteration is one E-step there
    (``expected_counts``) and the M-step on the host, in float64 and exactly

        a = (N01 + c01) / ((N00 + c00) + (N01 + c01)),   b = (N10 + c10) / ((N10 + c10) + (N11 + c11))

    with N the transition totals and c = ``prior_counts`` (c00, c01, c10, c11: pseudo-counts, a Dirichlet prior's exponents),
    each clamped to [1e-12, 1 - 1e-12]; a row without expected counts keeps its parameter.  ``p_start``: a float is kept
    fixed; 'free' starts at the stationary a / (a + b) and re-estimates it as G1 / (G0 + G1) (with one record that tends to 0
    or 1: meant for many records); 'stationary' ties it to a / (a + b) of every new a and b.  The loop stops when the log
    evidence L gains no more than ``tol`` max(1, |L|), or after ``max_iter`` M-steps.  A fixed or a free start is exact EM
    and, without prior counts, L never falls by more than rounding (with them it is L plus the log prior that rises).  The
    stationary start is a generalised step -- pi depends on a and b, which the M-step ignores -- and L need not be monotone:
    the loop stops at the first step that lowers L and returns the iterate before it, so the result is always the trace's
    best.  ``temper`` is not fitted (module docstring).  -> Fit."""
    x = evidence(scores, temper)
    return _fit(x, _offsets(owner_or_offsets, x.shape[0]), p_enter, p_leave, p_start, prior_counts, max_iter, tol, float(temper))


def default_temper(window, step, kmer_length):
    """min(1, step / (window - k + 1)): overlapping windows repeat the same k-mers window / step times, and tempering the
    evidence by the inverse is the composite-likelihood correction; exactly 1 for windows that do not overlap."""
    return min(1.0, float(step) / float(max(1, int(window) - int(kmer_length) + 1)))


class Segmentation(object):
    """What ``segment_track`` returns: the track's ``record_ids``, ``owner``, ``start``, ``window``, ``step``; the evidence
    ``x`` (n,); ``posterior``, ``state`` (n,); ``log_odds``, ``path_score`` (one per record id; 0 for a record without
    windows); and the parameters ``p_enter``, ``p_leave``, ``temper``."""

    def __init__(self, track, x, decoded, p_enter, p_leave, temper, fit=None):
        self.fit = fit     # the Fit whose values were decoded with (segment_track(fit=True)), else None
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


def _track_chain(track, mean_region, phage_fraction, temper, kmer_length):
    """(a, b, temper, x, offsets) of a track under ``segment_track``'s rules."""
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
    x = evidence(track.scores, t)
    records = len(track.record_ids)
    off = np.concatenate(([0], np.cumsum(np.bincount(track.owner, minlength=records)))).astype(np.uint64) \
        if len(track.owner) else np.zeros(records + 1, dtype=np.uint64)
    return a, b, t, x, off


def fit_track(track, mean_region=30000, phage_fraction=0.05, temper=None, kmer_length=4, p_start='stationary',
              prior_counts=(0, 0, 0, 0), max_iter=200, tol=1e-8):
    """``fit`` on a ``windows.WindowTrack``: ``mean_region`` and ``phage_fraction`` are the starting point, read as
    ``segment_track`` reads them; the Fit also carries what the fitted chain says of them, ``mean_region`` = step / p_leave
    and ``phage_fraction`` = a / (a + b).  ``temper`` as ``segment_track``; it is not fitted."""
    a, b, t, x, off = _track_chain(track, mean_region, phage_fraction, temper, kmer_length)
    return _fit(x, off, a, b, p_start, prior_counts, max_iter, tol, t, step=track.step)


def segment_track(track, mean_region=30000, phage_fraction=0.05, temper=None, kmer_length=4, fit=False, **fit_options):
    """Decodes a ``windows.WindowTrack``: p_leave = step / ``mean_region`` (the mean length of a phage region in bases;
    must be < 1), p_enter = p_leave * f / (1 - f) with f = ``phage_fraction`` (the stationary share of phage windows), the
    start distribution stationary.  ``temper=None``: ``default_temper(window, step, kmer_length)``.  The two defaults are
    modelling choices -- a prophage of tens of kb, a few per cent of a bacterial genome -- not measurements; ``fit=True``
    takes them as the starting point of ``fit_track`` (``fit_options``: its p_start, prior_counts, max_iter, tol) and decodes
    with the fitted p_enter, p_leave and p_start instead (``Segmentation.fit`` keeps the Fit).  The track may come from any
    method, but only ``likelihood`` and ``density`` scores are log-likelihood ratios.  -> Segmentation."""
    a, b, t, x, off = _track_chain(track, mean_region, phage_fraction, temper, kmer_length)
    if not fit:
        if fit_options:
            raise TypeError("%s only apply with fit=True" % sorted(fit_options))
        trans, init, qt, qp = parameters(a, b)
        return Segmentation(track, x, _decode(x, off, trans, init, qt, qp), a, b, t)
    fitted = _fit(x, off, a, b, fit_options.pop("p_start", 'stationary'), fit_options.pop("prior_counts", (0, 0, 0, 0)),
                  fit_options.pop("max_iter", 200), fit_options.pop("tol", 1e-8), t, step=track.step)
    if fit_options:
        raise TypeError("unknown fit options %s" % sorted(fit_options))
    trans, init, qt, qp = parameters(fitted.p_enter, fitted.p_leave, fitted.p_start)
    return Segmentation(track, x, _decode(x, off, trans, init, qt, qp), fitted.p_enter, fitted.p_leave, t, fit=fitted)


FIT_COLUMNS = "iteration,p_enter,p_leave,p_start,mean_region,phage_fraction,log_evidence"


def save_fit(filename, fitted, args=None):
    """``segment_fit.csv`` of a ``fit_track`` result: the '# ' comment header as ``save_segments`` writes it, then one line
    per trace row -- ``iteration,p_enter,p_leave,p_start,mean_region,phage_fraction,log_evidence``, floats by repr."""
    from . import fileIO, windows
    header = "PhaMers segment fit file"
    if args is not None:
        header = fileIO.generate_summary(args, header=header).rstrip('\n')
    rows = ["%d,%r,%r,%r,%r,%r,%r\n" % (i, float(r[0]), float(r[1]), float(r[2]), float(fitted.mean_regions[i]),
                                      float(fitted.phage_fractions[i]), float(r[9])) for i, r in enumerate(fitted.trace)]
    windows._write_csv(filename, header, FIT_COLUMNS, rows)


def read_fit(filename):
    """The rows of a file ``save_fit`` wrote: a list of (iteration, p_enter, p_leave, p_start, mean_region, phage_fraction,
    log_evidence)."""
    out = []
    with open(filename, 'r') as f:
        for line in f:
            if line.startswith('#') or not line.strip():
                continue
            v = line.rstrip('\n').split(',')
            out.append((int(v[0]),) + tuple(float(t) for t in v[1:]))
    return out


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
