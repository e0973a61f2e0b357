"""
compose.py -- reference-free segmentation of sequences by composition: an S-state hidden Markov chain whose states emit the
k-mer count rows of windows, fitted to the sequence itself by Baum-Welch (this project's own).

``windows`` scores windows against two references and ``segment`` decodes a two-state chain over such scores; ``mixture``
fits multinomial profiles to count rows but treats the rows as exchangeable.  Here neighbouring windows share a state:

    E[t][s]   = temper * sum_j c_t[j] log theta_s[j]              the emission of window t in state s (device, chain.hip)
    gamma, xi = the posteriors of the chain (A, pi) over E          forward-backward per record (device)
    T[s][j]   = sum_t gamma_t(s) c_t[j]     N_s = sum_t gamma_t(s)                          (device)
    theta_s   = (T_s + a) / (sum_j T_s[j] + D a)     A_ij = xi_ij / sum_j xi_ij             (``m_step``, NumPy)
    F         = L + a sum_s sum_j log theta_s[j]     L = the log evidence of the records    (what the loop raises)

The classic compositional segmentation of a genome (Churchill 1989; Nicolas et al. 2002): prophages, islands and chimeric
joins of a scaffold show as runs of another state, without a reference.  window = step (windows that do not overlap) is the
intended configuration; overlapping windows are tempered as ``segment.default_temper`` says.

Two findings of the CPU study this module was built after:
  * Starting from single random window rows (what ``mixture.start`` does) fails: on a 120 kb sequence of four pieces and
    three compositions every one of four seeds ended about 2300 nats below the right optimum with dozens of spurious
    regions.  ``start`` therefore pools blocks of consecutive windows and picks them farthest-first; it is the default.
  * A state too many does not stay empty: on a sequence of two compositions S = 3 splits off windows by sampling noise,
    because overlapping k-mers are over-dispersed against a multinomial.  S is the caller's choice; the evidence and a BIC
    are reported per fit and promise nothing, as in ``mixture.sweep``.

    start(counts, offsets, n_states, block, pseudocount)        (log_profiles (S, D), block indices)
    m_step(T, xi, gamma0, pseudocount, prior_counts, p_start)   (log_profiles, trans, init)
    fit(counts_or_batch, owner_or_offsets, n_states, ...)       a Composition
    segment_sequences(fasta_or_sequences, n_states, ...)        a ComposedSequences (fit + decode of the windows)
    load(path)                                                  a Composition saved with Composition.save
    fit_groups(counts_or_batch, owner_or_offsets, group_offsets, n_states, ...)
                                                                a Compositions: one fit per group of consecutive records,
                                                                all groups in one device call per iteration (section 4.28)
    load_groups(path)                                           a Compositions saved with Compositions.save
    boundary_plan(state, owner, start, window, step, span)      the intervals around the region boundaries of a decode;
                                                                ComposedSequences.refine / refined_regions: the boundaries
                                                                to the base (section 4.29; refine.py)
    python -m phamers_amd.compose -in FASTA -out DIR -S n [--scan [N]] [--per_record] [--refine [SPAN] [--confidence [NATS]]]
"""
import collections
import os

import numpy as np

from . import _lib
from .likelihood import _count_rows, _pseudocount
from .segment import QUANT_BITS, _offsets, default_temper, quantise

MAX_STATES = _lib.CHAIN_MAX_STATES
P_MIN = 1e-12
SCAN_FROM = 256    # ``scan=True``: records of at least this many windows take the tile scan (measured:
                   # profiles/compose_scan/README.md)
TRACE_COLUMNS = ("L", "F")

Decoded = collections.namedtuple("Decoded", "state posterior log_evidence path_score path_score_q")
Decoded.__doc__ = """state (n,) uint8, posterior (n, S) float64, log_evidence (R,) float64, path_score (R,) float64 nats
= path_score_q (R,) int64 * 2^-16."""


def _states(n_states):
    S = int(n_states)
    if not 2 <= S <= MAX_STATES:
        raise ValueError("n_states must be 2 to %d, got %r" % (MAX_STATES, n_states))
    return S


def _scan(scan):
    """``scan`` as a threshold in windows: None, False and 0 are 0 (no record takes the tile scan), True is ``SCAN_FROM``, an
    int >= 1 itself."""
    if scan is None or scan is False:
        return 0
    if scan is True:
        return SCAN_FROM
    if isinstance(scan, (int, np.integer)) and 0 <= int(scan) < 2 ** 64:
        return int(scan)
    raise ValueError("scan must be None, a bool or an int >= 0, got %r" % (scan,))


def _temper(temper):
    t = float(temper)
    if not (np.isfinite(t) and t > 0):
        raise ValueError("temper must be finite and > 0, got %r" % (temper,))
    return t


def _blocks(counts, offsets, block):
    """Pooled counts (n_blocks, D) int64 of every record's blocks of ``block`` consecutive windows."""
    block = int(block)
    if block < 1:
        raise ValueError("block must be >= 1, got %r" % (block,))
    off = [int(o) for o in np.asarray(offsets)]
    c = np.asarray(counts).astype(np.int64)
    rows = [c[s:min(s + block, b)].sum(axis=0) for a, b in zip(off[:-1], off[1:]) for s in range(a, b, block)]
    return np.array(rows, dtype=np.int64).reshape(len(rows), c.shape[1])


def _smooth(rows, a):
    rows = np.asarray(rows, dtype=np.float64)
    return np.log((rows + a) / (rows.sum(axis=1, keepdims=True) + rows.shape[1] * a))


def start(counts, offsets, n_states, block=20, pseudocount=0.5):
    """The deterministic start: every record is cut into blocks of ``block`` consecutive windows (never across records),
    their counts pooled, blocks without k-mers left out.  The first block is chosen; then, S - 1 times, the block whose
    best per-k-mer log-likelihood under the smoothed profiles of the chosen blocks is lowest (ties: the lowest index).
    (log_profiles (S, D) of the chosen blocks, their indices).  NumPy on the host."""
    c = _count_rows(counts, "counts")
    return _start(c, _offsets(offsets, len(c)), n_states, block, pseudocount)


def _start(c, offsets, n_states, block, pseudocount):
    S, a = _states(n_states), _pseudocount(pseudocount)
    P = _blocks(c, offsets, block)
    tot = P.sum(axis=1)
    live = np.flatnonzero(tot > 0)
    if len(live) < S:
        raise ValueError("n_states = %d exceeds the %d blocks of %d windows with k-mers" % (S, len(live), int(block)))
    Pl = P[live].astype(np.float64)
    chosen = [0]
    while len(chosen) < S:
        best = (Pl @ _smooth(Pl[chosen], a).T).max(axis=1) / tot[live]
        best[chosen] = np.inf
        chosen.append(int(np.argmin(best)))
    return _smooth(P[live[chosen]], a), [int(live[i]) for i in chosen]


def _normalised(v, keep):
    s = v.sum()
    if not s > 0:
        if keep is None:
            raise ValueError("a row without expected counts needs the values it keeps (trans= / init=)")
        return np.array(keep, dtype=np.float64)
    p = np.maximum(v / s, P_MIN)
    return p / p.sum()


def m_step(T, xi, gamma0, pseudocount, prior_counts=0.0, p_start='fixed', trans=None, init=None):
    """(log_profiles (S, D), trans (S, S), init) from the expected counts.  Profiles: ``mixture.m_step``'s formula.
    A_ij = (xi_ij + c_ij) / sum_j (xi_ij + c_ij) with c = ``prior_counts`` (a scalar or (S, S)), every entry raised to
    >= 1e-12 and the row divided by its sum again; a row whose denominator is 0 keeps ``trans``'s.  ``p_start='fixed'``
    returns ``init`` as it is, ``'free'`` gamma0 normalised and clamped the same way.  One NumPy operation per sign."""
    a = _pseudocount(pseudocount)
    T, xi = np.asarray(T, dtype=np.float64), np.asarray(xi, dtype=np.float64)
    if T.ndim != 2 or xi.shape != (T.shape[0], T.shape[0]):
        raise ValueError("T must be (S, D) and xi (S, S)")
    if p_start not in ('fixed', 'free'):
        raise ValueError("p_start must be 'fixed' or 'free'")
    S = T.shape[0]
    logp = np.log((T + a) / (T.sum(axis=1, keepdims=True) + T.shape[1] * a))
    x = xi + np.broadcast_to(np.asarray(prior_counts, dtype=np.float64), (S, S))
    A = np.array([_normalised(x[i], None if trans is None else np.asarray(trans)[i]) for i in range(S)])
    pi = init if p_start == 'fixed' else _normalised(np.asarray(gamma0, dtype=np.float64), init)
    return logp, A, pi


def start_chain(n_states, mean_region=30000, step=500):
    """(trans, init): 1 - step / mean_region on the diagonal, the rest shared equally; pi uniform."""
    S = _states(n_states)
    stay = 1.0 - float(step) / float(mean_region)
    if not 0.0 < stay < 1.0:
        raise ValueError("mean_region must exceed step")
    A = np.full((S, S), (1.0 - stay) / (S - 1))
    np.fill_diagonal(A, stay)
    return A, np.full(S, 1.0 / S)


class _DeviceEStep(object):
    """The device half of a fit or of a decode: the rows resident once in a ``_lib.Chain``."""

    def __init__(self, counts_or_batch, offsets, n_states, batch_rows=0):
        self.ctx = _lib.get_context()
        self.batch = counts_or_batch if isinstance(counts_or_batch, _lib.Batch) else None
        self.host = None if self.batch is not None else _count_rows(counts_or_batch, "counts")
        self.n = self.batch.n if self.batch is not None else len(self.host)
        self.D = self.batch.D if self.batch is not None else self.host.shape[1]
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)      # (resolved by the caller: _record_offsets)
        self.chain = _lib.Chain(self.ctx, self.batch if self.batch is not None else self.host, self.offsets, n_states, batch_rows)

    def counts(self):
        """uint32 count rows on the host (the start rule)."""
        if self.host is None:
            self.host = self.batch.counts_u32()
        return self.host

    def set_scan(self, scan_from):
        self.chain.set_scan(scan_from)

    def _set(self, log_profiles, trans, init, temper):
        self.chain.set(log_profiles, trans, init, quantise(np.log(trans)), quantise(np.log(init)), temper)

    def __call__(self, log_profiles, trans, init, temper):
        """(T, Ns, xi, gamma0, L) of one E-step."""
        self._set(log_profiles, trans, init, temper)
        return self.chain.expect()

    def decode(self, log_profiles, trans, init, temper):
        self._set(log_profiles, trans, init, temper)
        return self.chain.decode()

    def close(self):
        self.chain.close()


def _estep(counts_or_batch, offsets, n_states, batch_rows=0):
    """The E-step object of the rows (the tests put the statement in its place)."""
    return _DeviceEStep(counts_or_batch, offsets, n_states, batch_rows)


class _KnownOffsets(object):
    """Offsets (R + 1,) that are not to be read as owners whatever their length (segment_sequences)."""

    def __init__(self, offsets):
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)


def _record_offsets(counts_or_batch, owner_or_offsets):
    if isinstance(owner_or_offsets, _KnownOffsets):
        return owner_or_offsets.offsets
    n = counts_or_batch.n if isinstance(counts_or_batch, _lib.Batch) else len(_count_rows(counts_or_batch, "counts"))
    return _offsets(owner_or_offsets, n)


class Composition(object):
    """A fitted chain: ``log_profiles`` (S, D), ``trans`` (S, S), ``init`` (S,), ``temper``, ``pseudocount``; of the last
    E-step ``occupancy`` (N_s) and ``expected_counts`` (T); ``trace`` (iterates, 2): L and F; ``n_iter`` (M-steps),
    ``converged``, ``bic``.  A state with N_s = 0 has the uniform profile: ``empty`` (S,) bool reports it."""

    def __init__(self, log_profiles, trans, init, temper=1.0, pseudocount=0.5, occupancy=None, expected_counts=None, trace=None,
                 n_iter=0, converged=False, bic=np.nan):
        self.log_profiles = np.ascontiguousarray(log_profiles, dtype=np.float64)
        self.trans = np.ascontiguousarray(trans, dtype=np.float64)
        self.init = np.ascontiguousarray(init, dtype=np.float64)
        S = self.log_profiles.shape[0]
        if self.log_profiles.ndim != 2 or self.trans.shape != (S, S) or self.init.shape != (S,):
            raise ValueError("log_profiles must be (S, D), trans (S, S) and init (S,)")
        _states(S)
        self.temper, self.pseudocount = _temper(temper), float(pseudocount)
        self.occupancy = np.full(S, np.nan) if occupancy is None else np.asarray(occupancy, dtype=np.float64)
        self.expected_counts = (np.full(self.log_profiles.shape, np.nan) if expected_counts is None
                                else np.asarray(expected_counts, dtype=np.float64))
        self.trace = np.zeros((0, 2)) if trace is None else np.asarray(trace, dtype=np.float64).reshape(-1, 2)
        self.n_iter, self.converged, self.bic = int(n_iter), bool(converged), float(bic)

    @property
    def n_states(self):
        return self.log_profiles.shape[0]

    @property
    def empty(self):
        return self.occupancy == 0

    def decode(self, counts_or_batch, owner_or_offsets, scan=None):
        """The Viterbi path, the posteriors (n, S), the log evidence per record and the path score of count rows (or a
        resident batch) cut into records by ``owner_or_offsets`` (see ``segment.decode``): a ``Decoded``.  ``scan``: the
        records that take the tile scan (see ``fit``); their path and path score are the same bits either way."""
        scan = _scan(scan)
        offsets = _record_offsets(counts_or_batch, owner_or_offsets)
        estep = _estep(counts_or_batch, offsets, self.n_states)
        try:
            if scan:
                estep.set_scan(scan)
            if estep.D != self.log_profiles.shape[1]:
                raise ValueError("the counts have %d columns, the composition %d" % (estep.D, self.log_profiles.shape[1]))
            state, post, le, ps = estep.decode(self.log_profiles, self.trans, self.init, self.temper)
        finally:
            estep.close()
        return Decoded(state, post, le, ps.astype(np.float64) * 2.0 ** -QUANT_BITS, ps)

    def label(self, positive_counts, negative_counts):
        """(S,) float64: ``likelihood.score(..., per_kmer=True)`` of every state's rint(T_s) row against the two
        references -- positive for a state whose composition is the positive class's (nan for an empty state)."""
        from . import likelihood
        rows = np.rint(self.expected_counts)
        if not np.isfinite(rows).all():
            raise ValueError("this composition has no expected counts (it was not fitted)")
        return likelihood.score(rows.astype(np.uint32), positive_counts, negative_counts, self.pseudocount, per_kmer=True)

    def save(self, path):
        """A ``.npz`` file that ``load`` reads back."""
        with open(path, 'wb') as f:
            np.savez(f, log_profiles=self.log_profiles, trans=self.trans, init=self.init, temper=self.temper,
                     pseudocount=self.pseudocount, occupancy=self.occupancy, expected_counts=self.expected_counts,
                     trace=self.trace, n_iter=self.n_iter, converged=self.converged, bic=self.bic)


def load(path):
    """The Composition of a file written by ``Composition.save``."""
    with np.load(path) as z:
        return Composition(z["log_profiles"], z["trans"], z["init"], float(z["temper"]), float(z["pseudocount"]), z["occupancy"],
                           z["expected_counts"], z["trace"], int(z["n_iter"]), bool(z["converged"]), float(z["bic"]))


def _initial_profiles(estep, S, init, block, a):
    if init is None:
        return _start(estep.counts(), estep.offsets, S, block, a)[0]
    init = np.asarray(init)
    if init.ndim == 2:
        p = np.asarray(init, dtype=np.float64)
        if p.shape != (S, estep.D) or not (np.isfinite(p).all() and (p > 0).all()):
            raise ValueError("init profiles must be (%d, %d), finite and > 0" % (S, estep.D))
        return np.log(p / p.sum(axis=1, keepdims=True))
    P = _blocks(estep.counts(), estep.offsets, block)
    if init.shape != (S,) or not np.issubdtype(init.dtype, np.integer) or init.min() < 0 or init.max() >= len(P):
        raise ValueError("init must be %d block indices below %d, or (S, D) profiles" % (S, len(P)))
    return _smooth(P[init], a)


def fit(counts_or_batch, owner_or_offsets, n_states, mean_region=30000, step=500, temper=1.0, pseudocount=0.5, init=None,
        block=20, prior_counts=0, fit_transitions=True, p_start='fixed', max_iter=100, tol=1e-6, scan=None):
    """An S-state chain fitted by Baum-Welch to the count rows ``counts_or_batch`` ((n, D) integers, made resident once, or
    a ``_lib.Batch``, read where it lies) cut into records by ``owner_or_offsets`` (see ``segment.decode``).  The profiles
    start from ``start`` (``init``: S block indices or (S, D) profiles instead), the chain from ``start_chain``.  The loop
    is ``mixture``'s: it stops at the first iterate with F_i - F_{i-1} <= tol max(1, |F_i|) or after ``max_iter`` M-steps.
    ``fit_transitions=False`` keeps the start chain.  gamma and E never leave the device.  ``scan``: None, False or 0 keep
    every record on the per-record route; True sends the records of at least ``SCAN_FROM`` windows, an int >= 1 those of at
    least that many, through the tile scan, which works on a long record in parallel and gives
    its expectations within that section's bound.  A ``Composition``."""
    S, a, t = _states(n_states), _pseudocount(pseudocount), _temper(temper)
    scan = _scan(scan)
    max_iter, tol = int(max_iter), float(tol)
    if max_iter < 0 or not (np.isfinite(tol) and tol >= 0):
        raise ValueError("max_iter >= 0 and a finite tol >= 0 are required")
    if p_start not in ('fixed', 'free'):
        raise ValueError("p_start must be 'fixed' or 'free'")
    A, pi = start_chain(S, mean_region, step)
    offsets = _record_offsets(counts_or_batch, owner_or_offsets)
    estep = _estep(counts_or_batch, offsets, S)
    try:
        if scan:
            estep.set_scan(scan)
        logp = _initial_profiles(estep, S, init, block, a)
        trace, F_prev, converged = [], None, False
        for it in range(max_iter + 1):
            T, Ns, xi, g0, L = estep(logp, A, pi, t)
            F = float(L) + a * float(np.sum(logp))
            trace.append((L, F))
            if F_prev is not None and F - F_prev <= tol * max(1.0, abs(F)):
                converged = True
                break
            if it == max_iter:
                break
            F_prev = F
            logp, A2, pi2 = m_step(T, xi, g0, a, prior_counts, p_start, A, pi)
            if fit_transitions:
                A, pi = A2, pi2
        n = estep.n
    finally:
        estep.close()
    free = S * (logp.shape[1] - 1) + (S * (S - 1) if fit_transitions else 0) + (S - 1 if p_start == 'free' else 0)
    bic = -2.0 * float(trace[-1][0]) + free * float(np.log(max(n, 1)))
    return Composition(logp, A, pi, t, a, Ns, T, np.array(trace, dtype=np.float64), len(trace) - 1, converged, bic)


# ---- one fit per group of records ---------------------------------------------------------------------
GROUP_FITTED, GROUP_TOO_SHORT = 0, 1     # ``Compositions.status``


class _DeviceGroupEStep(object):
    """The device half of ``fit_groups`` and ``Compositions.decode``: the rows resident once in a grouped ``_lib.Chain``."""

    def __init__(self, counts_or_batch, offsets, group_offsets, n_states, batch_rows=0):
        self.base = _DeviceEStep(counts_or_batch, offsets, n_states, batch_rows)
        self.n, self.D, self.offsets = self.base.n, self.base.D, self.base.offsets
        self.group_offsets = np.ascontiguousarray(group_offsets, dtype=np.uint64)
        try:
            self.base.chain.set_groups(self.group_offsets)
        except Exception:
            self.base.close()
            raise

    def counts(self):
        return self.base.counts()

    def _set(self, log_profiles, trans, init, temper, active):
        tr, pi = np.asarray(trans, dtype=np.float64), np.asarray(init, dtype=np.float64)
        self.base.chain.set_grouped(log_profiles, tr, pi, quantise(np.log(tr)), quantise(np.log(pi)), temper, active)

    def __call__(self, log_profiles, trans, init, temper, active):
        """(T (G, S, D), Ns, xi, gamma0, L (G,)) of one E-step of the active groups (zeros for the others)."""
        self._set(log_profiles, trans, init, temper, active)
        return self.base.chain.expect_grouped()

    def decode(self, log_profiles, trans, init, temper, active):
        self._set(log_profiles, trans, init, temper, active)
        return self.base.chain.decode()

    def close(self):
        self.base.close()


def _estep_groups(counts_or_batch, offsets, group_offsets, n_states, batch_rows=0):
    """The grouped E-step object of the rows (the tests put the statement in its place)."""
    return _DeviceGroupEStep(counts_or_batch, offsets, group_offsets, n_states, batch_rows)


def _group_offsets(group_offsets, n_records):
    go = np.asarray(group_offsets)
    if go.ndim != 1 or len(go) < 1 or not np.issubdtype(go.dtype, np.integer):
        raise ValueError("group_offsets must be (G + 1,) integers")
    go = go.astype(np.int64)
    if go[0] != 0 or go[-1] != n_records or (np.diff(go) < 0).any():
        raise ValueError("group_offsets must run from 0 to the %d records and never decrease" % n_records)
    return go.astype(np.uint64)


class _GroupRows(object):
    """The rows of one group as ``_initial_profiles`` reads them: its count rows and its own record offsets."""

    def __init__(self, rows, offsets, D):
        self.rows, self.offsets, self.D = rows, offsets, D

    def counts(self):
        return self.rows


def _group_rows(counts, offsets, group_offsets, g, D):
    r0, r1 = int(group_offsets[g]), int(group_offsets[g + 1])
    off = np.asarray(offsets[r0:r1 + 1]).astype(np.int64)
    return _GroupRows(counts[int(off[0]):int(off[-1])], (off - off[0]).astype(np.uint64), D)


def group_status(rows, offsets, n_states, block):
    """``GROUP_TOO_SHORT`` for rows whose records hold fewer than ``n_states`` blocks of ``block`` windows with k-mers
    (``start`` has nothing to choose from; ``fit`` raises for them), else ``GROUP_FITTED``."""
    live = int((_blocks(rows, offsets, block).sum(axis=1) > 0).sum()) if len(rows) else 0
    return GROUP_TOO_SHORT if live < n_states else GROUP_FITTED


class Compositions(object):
    """What ``fit_groups`` returns: one fitted chain per group of records.  ``len`` and ``[g]`` (a ``Composition``, or None
    for a group that was not fitted); stacked over the groups ``log_profiles`` (G, S, D), ``trans`` (G, S, S), ``init``
    (G, S), ``occupancy`` (G, S), ``expected_counts`` (G, S, D), ``n_iter``, ``converged``, ``bic`` and ``status`` (G,)
    (``GROUP_FITTED`` or ``GROUP_TOO_SHORT``; a group that was not fitted has NaN parameters); ``traces``: a list of
    (iterates, 2) arrays.  State numbers are a group's own: state 1 of one group and state 1 of another have nothing to
    do with each other (``label`` scores every state against two references, which is comparable)."""

    def __init__(self, compositions, status, n_states, n_columns, temper=1.0, pseudocount=0.5):
        self._items = list(compositions)
        self.status = np.asarray(status, dtype=np.int64).reshape(len(self._items))
        self.n_states, self.n_columns = _states(n_states), int(n_columns)
        self.temper, self.pseudocount = _temper(temper), float(pseudocount)
        G, S, D = len(self._items), self.n_states, self.n_columns
        for c in self._items:
            if c is not None and c.log_profiles.shape != (S, D):
                raise ValueError("every composition must be (%d, %d)" % (S, D))
        stack = lambda name, shape: np.array([np.full(shape, np.nan) if c is None else getattr(c, name) for c in self._items],
                                             dtype=np.float64).reshape((G,) + shape)
        self.log_profiles, self.expected_counts = stack("log_profiles", (S, D)), stack("expected_counts", (S, D))
        self.trans, self.init, self.occupancy = stack("trans", (S, S)), stack("init", (S,)), stack("occupancy", (S,))
        self.bic = stack("bic", ())
        self.n_iter = np.array([0 if c is None else c.n_iter for c in self._items], dtype=np.int64)
        self.converged = np.array([False if c is None else c.converged for c in self._items], dtype=bool)
        self.traces = [np.zeros((0, 2)) if c is None else c.trace for c in self._items]

    def __len__(self):
        return len(self._items)

    def __getitem__(self, g):
        return self._items[g]

    @property
    def fitted(self):
        """(G,) bool: the groups that have a Composition."""
        return np.array([c is not None for c in self._items], dtype=bool)

    def decode(self, counts_or_batch, owner_or_offsets, group_offsets):
        """Every record decoded with its group's chain, all groups in one device call: a ``Decoded`` over all the windows
        and records.  The records of a group that was not fitted get state 0, NaN posteriors, NaN evidence and NaN path
        score (path_score_q 0)."""
        offsets = _record_offsets(counts_or_batch, owner_or_offsets)
        go = _group_offsets(group_offsets, len(offsets) - 1)
        if len(go) - 1 != len(self):
            raise ValueError("%d groups, %d compositions" % (len(go) - 1, len(self)))
        S, fitted = self.n_states, self.fitted
        estep = _estep_groups(counts_or_batch, offsets, go, S)
        try:
            if estep.D != self.n_columns:
                raise ValueError("the counts have %d columns, the compositions %d" % (estep.D, self.n_columns))
            A0, pi0 = start_chain(S)
            logp = np.where(fitted[:, None, None], self.log_profiles, 0.0)
            A, pi = np.where(fitted[:, None, None], self.trans, A0), np.where(fitted[:, None], self.init, pi0)
            state, post, le, ps = estep.decode(logp, A, pi, self.temper, fitted)
        finally:
            estep.close()
        score = ps.astype(np.float64) * 2.0 ** -QUANT_BITS
        off = offsets.astype(np.int64)
        for g in np.flatnonzero(~fitted):
            r0, r1 = int(go[g]), int(go[g + 1])
            state[off[r0]:off[r1]], post[off[r0]:off[r1]] = 0, np.nan
            le[r0:r1], score[r0:r1], ps[r0:r1] = np.nan, np.nan, 0
        return Decoded(state, post, le, score, ps)

    def label(self, positive_counts, negative_counts):
        """(G, S) float64: ``Composition.label`` of every group -- every state's rint(T_s) row scored against the two
        references, which is comparable between groups where state numbers are not (NaN for a group that was not fitted)."""
        from . import likelihood
        out = np.full((len(self), self.n_states), np.nan)
        fitted = np.flatnonzero(self.fitted)
        if len(fitted):
            rows = np.rint(self.expected_counts[fitted]).reshape(-1, self.n_columns)
            out[fitted] = likelihood.score(rows.astype(np.uint32), positive_counts, negative_counts, self.pseudocount,
                                           per_kmer=True).reshape(len(fitted), self.n_states)
        return out

    def save(self, path):
        """A ``.npz`` file that ``load_groups`` reads back."""
        ends = np.cumsum([0] + [len(t) for t in self.traces])
        trace = np.concatenate(self.traces).reshape(-1, 2) if len(self.traces) else np.zeros((0, 2))
        with open(path, 'wb') as f:
            np.savez(f, log_profiles=self.log_profiles, trans=self.trans, init=self.init, temper=self.temper,
                     pseudocount=self.pseudocount, occupancy=self.occupancy, expected_counts=self.expected_counts, trace=trace,
                     trace_offsets=ends, n_iter=self.n_iter, converged=self.converged, bic=self.bic, status=self.status,
                     n_states=self.n_states, n_columns=self.n_columns)


def load_groups(path):
    """The Compositions of a file written by ``Compositions.save``."""
    with np.load(path) as z:
        t, a, ends = float(z["temper"]), float(z["pseudocount"]), z["trace_offsets"]
        items = [None if z["status"][g] != GROUP_FITTED else
                 Composition(z["log_profiles"][g], z["trans"][g], z["init"][g], t, a, z["occupancy"][g], z["expected_counts"][g],
                             z["trace"][ends[g]:ends[g + 1]], int(z["n_iter"][g]), bool(z["converged"][g]), float(z["bic"][g]))
                 for g in range(len(z["status"]))]
        return Compositions(items, z["status"], int(z["n_states"]), int(z["n_columns"]), t, a)


def fit_groups(counts_or_batch, owner_or_offsets, group_offsets, n_states, mean_region=30000, step=500, temper=1.0,
               pseudocount=0.5, init=None, block=20, prior_counts=0, fit_transitions=True, p_start='fixed', max_iter=100,
               tol=1e-6, **options):
    """One ``fit`` per group of records, all groups side by side: the records (``owner_or_offsets`` as in ``fit``) are cut
    into G groups of consecutive records by ``group_offsets`` (G + 1,) -- a scaffold, or the scaffolds of a bin --, every
    group has its own profiles, transition matrix and start vector, and every Baum-Welch iteration is one device call for
    all the groups that have not stopped.  Per group the start rule (``start`` on the group's own
    records), ``start_chain``, ``m_step``, the stop rule and ``max_iter`` are ``fit``'s, and the group's ``Composition``
    is bit for bit what ``fit`` gives on the group's records alone.  ``init``: as in ``fit`` for every group, or a list
    with one entry per group.  A group with fewer than ``n_states`` blocks with k-mers (``fit`` raises for it) is not
    fitted: status ``GROUP_TOO_SHORT``, NaN parameters, no device work.  The tile scan is not available here (``scan``
    raises ValueError).  A ``Compositions``."""
    if "scan" in options:
        raise ValueError("fit_groups does not take the tile scan (scan=): a grouped chain runs the per-record route")
    if options:
        raise TypeError("fit_groups() got unexpected arguments %s" % sorted(options))
    S, a, t = _states(n_states), _pseudocount(pseudocount), _temper(temper)
    max_iter, tol = int(max_iter), float(tol)
    if max_iter < 0 or not (np.isfinite(tol) and tol >= 0):
        raise ValueError("max_iter >= 0 and a finite tol >= 0 are required")
    if p_start not in ('fixed', 'free'):
        raise ValueError("p_start must be 'fixed' or 'free'")
    A0, pi0 = start_chain(S, mean_region, step)
    offsets = _record_offsets(counts_or_batch, owner_or_offsets)
    go = _group_offsets(group_offsets, len(offsets) - 1)
    G = len(go) - 1
    inits = list(init) if isinstance(init, list) else [init] * G
    if len(inits) != G:
        raise ValueError("init lists %d groups of %d" % (len(inits), G))
    estep = _estep_groups(counts_or_batch, offsets, go, S)
    try:
        D, counts = estep.D, estep.counts()
        status = np.zeros(G, dtype=np.int64)
        logp, A, pi = [np.zeros((S, D))] * G, [A0] * G, [pi0] * G
        n_windows = np.zeros(G, dtype=np.int64)
        for g in range(G):
            rows = _group_rows(counts, offsets, go, g, D)
            n_windows[g] = len(rows.rows)
            status[g] = group_status(rows.rows, rows.offsets, S, block)
            if status[g] == GROUP_FITTED:
                logp[g] = _initial_profiles(rows, S, inits[g], block, a)
        active = status == GROUP_FITTED
        traces, F_prev = [[] for _ in range(G)], [None] * G
        converged, T_last, Ns_last = np.zeros(G, dtype=bool), [None] * G, [None] * G
        for it in range(max_iter + 1):
            if not active.any():
                break
            T, Ns, xi, g0, L = estep(np.array(logp), np.array(A), np.array(pi), t, active)
            for g in np.flatnonzero(active):
                F = float(L[g]) + a * float(np.sum(logp[g]))
                traces[g].append((float(L[g]), F))
                T_last[g], Ns_last[g] = T[g], Ns[g]
                if F_prev[g] is not None and F - F_prev[g] <= tol * max(1.0, abs(F)):
                    converged[g], active[g] = True, False     # (a group that has stopped drops out of the later calls)
                    continue
                if it == max_iter:
                    active[g] = False
                    continue
                F_prev[g] = F
                logp[g], A2, pi2 = m_step(T[g], xi[g], g0[g], a, prior_counts, p_start, A[g], pi[g])
                if fit_transitions:
                    A[g], pi[g] = A2, pi2
    finally:
        estep.close()
    free = S * (D - 1) + (S * (S - 1) if fit_transitions else 0) + (S - 1 if p_start == 'free' else 0)
    items = []
    for g in range(G):
        if status[g] != GROUP_FITTED:
            items.append(None)
            continue
        bic = -2.0 * float(traces[g][-1][0]) + free * float(np.log(max(int(n_windows[g]), 1)))
        items.append(Composition(logp[g], A[g], pi[g], t, a, Ns_last[g].copy(), T_last[g].copy(), np.array(traces[g], dtype=np.float64),
                                 len(traces[g]) - 1, bool(converged[g]), bic))
    return Compositions(items, status, S, D, t, a)


# ---- boundaries finer than a window ---------------------------------------------------------------
BoundaryPlan = collections.namedtuple("BoundaryPlan", "record x lo hi left_state right_state first_window")
BoundaryPlan.__doc__ = """One entry per pair of adjacent runs of a record, in window order, all (B,) int64: the record, the
window boundary x, the interval lo .. hi in bases of the record, the two runs' states and the index of the right run's
first window."""

Boundaries = collections.namedtuple("Boundaries", "record record_id window_boundary position left_state right_state gain "
                                                  "left_evidence right_evidence support evidence_q")
Boundaries.__doc__ = """What ``ComposedSequences.refine`` fills, one entry per boundary: the record (index and id), the window
boundary x, the refined position, the two states, gain / left_evidence / right_evidence in nats (float64) -- ``evidence_q``
(B, 3) int64 holds the same three in units of 2^-16 nat, exact -- and the support (valid k-mers of the interval)."""


def _runs(state, owner):
    """(first, last) window index of every run of consecutive windows of one record in one state."""
    joined = (state[1:] == state[:-1]) & (owner[1:] == owner[:-1])
    return np.flatnonzero(np.concatenate(([True], ~joined))), np.flatnonzero(np.concatenate((~joined, [True])))


def boundary_plan(state, owner, start, window, step, span=None):
    """The intervals in which the boundaries of a decode are looked for: one per pair of adjacent runs A = windows a0 .. a1,
    B = windows b0 .. b1 of one record (runs of different records are never joined).  With integer division throughout:

        x         = (start[a1] + window + start[b0]) // 2        the window boundary (start[b0] when window = step)
        left_mid  = (start[a0] + start[a1] + window) // 2        the middle of run A; right_mid likewise of run B
        lo        = min(x, max(x - span, left_mid + 1))
        hi        = max(x, min(x + span, right_mid))

    ``span`` defaults to ``window``.  The middle of a run is at least the hi of the boundary before it and below the lo of
    the one after it, so the intervals of a record are disjoint and, whatever position is chosen inside them, the refined
    positions of a record increase strictly: no refined region is empty or out of order.  (This needs
    (window + step) // 2 > window // 2, that is step >= 2 or an odd window; with step = 1 and an even window the two
    intervals around a run of a single window share their end point.)  The formulas read the window starts; ``step`` is
    only checked.  A ``BoundaryPlan``.  NumPy on the host."""
    state, owner = np.asarray(state).astype(np.int64).reshape(-1), np.asarray(owner).astype(np.int64).reshape(-1)
    start = np.asarray(start).astype(np.int64).reshape(-1)
    window, step = int(window), int(step)
    if window < 1 or step < 1:
        raise ValueError("window and step must be >= 1")
    span = window if span is None else int(span)
    if span < 0:
        raise ValueError("span must be >= 0, got %r" % (span,))
    if not len(state) == len(owner) == len(start):
        raise ValueError("state, owner and start must have one entry per window")
    empty = np.zeros(0, dtype=np.int64)
    if len(state) == 0:
        return BoundaryPlan(*([empty] * 7))
    first, last = _runs(state, owner)
    pair = np.flatnonzero(owner[first[:-1]] == owner[first[1:]])
    a0, a1, b0, b1 = first[pair], last[pair], first[pair + 1], last[pair + 1]
    x = (start[a1] + window + start[b0]) // 2
    left_mid = (start[a0] + start[a1] + window) // 2
    right_mid = (start[b0] + start[b1] + window) // 2
    lo = np.minimum(x, np.maximum(x - span, left_mid + 1))
    hi = np.maximum(x, np.minimum(x + span, right_mid))
    return BoundaryPlan(owner[a0], x, lo, hi, state[a0], state[b0], b0)


def _span(refine):
    """``refine`` of ``segment_sequences``: False / None = no, True = the default span (None), an int >= 0 = that span."""
    if isinstance(refine, (bool, np.bool_)) or refine is None:
        return bool(refine), None
    if isinstance(refine, (int, np.integer)) and int(refine) >= 0:
        return True, int(refine)
    raise ValueError("refine must be a bool or a span in bases >= 0, got %r" % (refine,))


def _drop(confidence):
    """``confidence`` of ``ComposedSequences.refine``: None / False = no, True = ``refine.DEFAULT_DROP`` nats, a number >= 0 =
    that many nats.  None or the drop as a float."""
    from . import refine as _refine
    if confidence is None or (isinstance(confidence, (bool, np.bool_)) and not confidence):
        return None
    if isinstance(confidence, (bool, np.bool_)):
        return _refine.DEFAULT_DROP
    if isinstance(confidence, (int, float, np.integer, np.floating)):
        _refine.drop_quantum(confidence)
        return float(confidence)
    raise ValueError("confidence must be a bool or a number of nats >= 0, got %r" % (confidence,))


class ComposedSequences(object):
    """What ``segment_sequences`` returns: ``composition``; the windows' ``record_ids``, ``owner``, ``start``, ``window``,
    ``step``; ``state`` (n,), ``posterior`` (n, S); ``log_evidence`` and ``path_score`` per record; ``boundaries``: None until
    ``refine`` has run, then a ``Boundaries``; ``boundary_confidence``: None until ``refine(confidence=...)`` has run, then a
    ``refine.Confidence`` with one entry per entry of ``boundaries``."""

    def __init__(self, composition, record_ids, owner, start, window, step, decoded):
        self.composition, self.record_ids, self.owner, self.start = composition, list(record_ids), owner, start
        self.window, self.step = int(window), int(step)
        self.state, self.posterior = decoded.state, decoded.posterior
        self.log_evidence, self.path_score = decoded.log_evidence, decoded.path_score
        self.boundaries = None
        self.boundary_confidence = None

    def __len__(self):
        return self.state.shape[0]

    def refine(self, fasta_or_sequences, span=None, confidence=None):
        """Refines every boundary between two runs of a record from the window grid to the base (``refine.boundaries`` on
        the intervals of ``boundary_plan``; ``span``: bases searched on either side of a window boundary at most, default
        ``window``) and fills ``self.boundaries``.  ``fasta_or_sequences`` is the input the windows were counted from.  The
        two states' profiles are row s of a ``Composition``'s ``log_profiles``, or row g S + s of a ``Compositions``' for
        record g (one group per record, as ``segment_sequences(per_record=True)`` fits them); a record whose group was not
        fitted is one run of state 0 and has no boundary.  A composition fitted with ``both_strands`` has folded
        (strand-symmetric) profiles; they are used as they are, with the forward strand's k-mers.  Returns ``self``.

        ``confidence``: True, or a drop in nats, also fills ``self.boundary_confidence`` (``refine.confidence``: a support
        interval and the position's posterior per boundary; True = 3 nats); None or False leaves it
        None and is the call without it.  ``boundaries`` and ``refined_regions()`` are the same either way."""
        from . import refine as _refine
        drop = _drop(confidence)
        comp = self.composition
        grouped = isinstance(comp, Compositions)
        D = comp.n_columns if grouped else comp.log_profiles.shape[1]
        k = int(round(np.log(D) / np.log(4)))
        plan = boundary_plan(self.state, self.owner, self.start, self.window, self.step, span)
        S = comp.n_states
        if grouped:
            table = np.where(np.isnan(comp.log_profiles), 0.0, comp.log_profiles).reshape(-1, D)
            left, right = plan.record * S + plan.left_state, plan.record * S + plan.right_state
        else:
            table, left, right = comp.log_profiles, plan.left_state, plan.right_state
        if drop is None:
            r = _refine.boundaries(fasta_or_sequences, k, table, plan.record, plan.lo, plan.x, plan.hi, left, right)
            self.boundary_confidence = None
        else:
            r, self.boundary_confidence = _refine.confidence(fasta_or_sequences, k, table, plan.record, plan.lo, plan.x, plan.hi,
                                                             left, right, drop)
        self.boundaries = Boundaries(plan.record, [self.record_ids[int(g)] for g in plan.record], plan.x, r.position,
                                     plan.left_state, plan.right_state, r.gain_nats, r.left_evidence_nats, r.right_evidence_nats,
                                     r.support, np.stack([r.gain, r.left_evidence, r.right_evidence], axis=1).reshape(-1, 3))
        return self

    def refined_regions(self):
        """``regions()`` with the start and the end of every region that borders another region of its record replaced by
        the refined position of that boundary; a record's first start and last end stay.  ValueError before ``refine``."""
        if self.boundaries is None:
            raise ValueError("refined_regions needs the boundaries: call refine(fasta_or_sequences) first")
        regions = [list(r) for r in self.regions()]
        if regions:
            first, _ = _runs(self.state, self.owner)
            pair = np.flatnonzero(self.owner[first[:-1]] == self.owner[first[1:]])
            if len(pair) != len(self.boundaries.position):
                raise ValueError("the boundaries do not belong to this decode")
            for r, p in zip(pair, self.boundaries.position):
                regions[int(r)][2] = regions[int(r) + 1][1] = int(p)
        return [tuple(r) for r in regions]

    def regions(self):
        """Per run of consecutive windows of one record in one state: ``(record id, start of the first window, start of the
        last + window, state, n_windows, mean posterior of that state)``, ordered by record and start."""
        n = len(self)
        if n == 0:
            return []
        joined = (self.state[1:] == self.state[:-1]) & (self.owner[1:] == self.owner[:-1])
        first = np.flatnonzero(np.concatenate(([True], ~joined)))
        last = np.flatnonzero(np.concatenate((~joined, [True])))
        return [(self.record_ids[int(self.owner[a])], int(self.start[a]), int(self.start[b]) + self.window, int(self.state[a]),
                 int(b - a + 1), float(self.posterior[a:b + 1, int(self.state[a])].mean())) for a, b in zip(first, last)]


def segment_sequences(fasta_or_sequences, n_states, window=500, step=500, kmer_length=4, both_strands=False, scan=None,
                      per_record=False, refine=False, confidence=None, **fit_options):
    """Counts the windows of a FASTA file (or a list of strings) as one resident batch, fits ``n_states`` compositions to
    them and decodes: a ``ComposedSequences``.  ``temper`` defaults to ``segment.default_temper(window, step, k)``; the other
    ``fit_options`` are ``fit``'s (``step`` is passed on); ``scan`` goes to the fit and to the decode.  ValueError when no
    sequence holds a window.

    ``per_record=True`` fits one chain per record instead (``fit_groups`` with one group per record: a prophage or island
    then stands out against its own scaffold, not against the other organisms of an assembly); ``composition`` is then
    the ``Compositions``.  State numbers are then NOT comparable between records -- state 1 of one record and state 1 of
    another are unrelated; ``Compositions.label`` scores every (record, state) against two references, which is.  A record
    too short for ``n_states`` is not fitted (state 0, NaN posteriors).  ``per_record`` does not go with ``scan``.

    ``refine``: True, or a span in bases, refines the region boundaries to the base before returning
    (``ComposedSequences.refine`` with this call's input); False leaves ``boundaries`` None.
    ``confidence`` (True, or a drop in nats) is passed to that call and fills ``boundary_confidence`` (section 4.30); it
    requires ``refine``."""
    from . import kmer
    scan = _scan(scan)
    refine, span = _span(refine)
    if _drop(confidence) is not None and not refine:
        raise ValueError("confidence requires refine")
    if per_record and scan:
        raise ValueError("per_record does not go with the tile scan (scan=)")
    both_strands = kmer._check_strands(kmer.DNA, both_strands)
    record_ids, lengths, batch = kmer._windows_batch(fasta_or_sequences, kmer_length, window, step)
    if batch is None:
        raise ValueError("no sequence is as long as the window (%d)" % int(window))
    try:
        if both_strands:
            batch.fold_strands()
        owner, first = kmer.window_plan(lengths, window, step)
        fit_options.setdefault("temper", default_temper(window, step, kmer_length))
        offsets = _KnownOffsets(np.concatenate(([0], np.cumsum(np.bincount(owner, minlength=len(record_ids))))))
        if per_record:
            groups = np.arange(len(record_ids) + 1, dtype=np.uint64)
            comp = fit_groups(batch, offsets, groups, n_states, step=step, **fit_options)
            decoded = comp.decode(batch, offsets, groups)
        else:
            comp = fit(batch, offsets, n_states, step=step, scan=scan, **fit_options)
            decoded = comp.decode(batch, offsets, scan=scan)
    finally:
        batch.close()
    result = ComposedSequences(comp, record_ids, owner, first, window, step, decoded)
    return result.refine(fasta_or_sequences, span, confidence) if refine else result


# ---- command line ---------------------------------------------------------------------------------------------------------
def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="Segment sequences by composition: an S-state chain fitted to their windows",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument('-in', '--input_file', required=True, help="FASTA file")
    ap.add_argument('-out', '--output_directory', required=True, help="Directory of the four CSV files")
    ap.add_argument('-S', '--states', type=int, required=True, help="States of the chain (2 to 8)")
    ap.add_argument('-w', '--window', type=int, default=500, help="Window length in bases")
    ap.add_argument('-s', '--step', type=int, default=500, help="Bases between window starts (window = step is intended)")
    ap.add_argument('-k', '--kmer_length', type=int, default=4, help="k-mer length")
    ap.add_argument('--both_strands', action='store_true', help="Count every window with its reverse complement")
    ap.add_argument('--mean_region', type=float, default=30000, help="Mean region length in bases of the start chain")
    ap.add_argument('--temper', type=float, default=None, help="Exponent of the emissions (default: by window and step)")
    ap.add_argument('--block', type=int, default=20, help="Windows per block of the start rule")
    ap.add_argument('--max_iter', type=int, default=100, help="Most M-steps")
    ap.add_argument('--tol', type=float, default=1e-6, help="Relative gain of the evidence below which the loop stops")
    ap.add_argument('--keep_transitions', action='store_true', help="Do not fit the transition probabilities")
    ap.add_argument('--scan', type=int, nargs='?', const=True, default=None, metavar='N',
                    help="Work on records of at least N windows in parallel by the tile scan (without N: %d)" % SCAN_FROM)
    ap.add_argument('--per_record', action='store_true',
                    help="Fit one chain per record (state numbers are then a record's own; not with --scan)")
    ap.add_argument('--refine', type=int, nargs='?', const=True, default=None, metavar='SPAN',
                    help="Refine the region boundaries to the base, searching SPAN bases on either side of a window boundary "
                         "(without SPAN: the window); writes compose_boundaries.csv and compose_segments_refined.csv")
    ap.add_argument('--confidence', type=float, nargs='?', const=True, default=None, metavar='NATS',
                    help="With --refine: per boundary the support interval of the positions within NATS of the best log "
                         "likelihood (without NATS: 3) and the position's posterior; writes compose_boundary_confidence.csv")
    ap.add_argument('-pf', '--positive_features', default=None, help="Count file of the positive reference (labels the states)")
    ap.add_argument('-nf', '--negative_features', default=None, help="Count file of the negative reference")
    return ap


def _write_record_files(directory, result, phage_score):
    """compose_profiles.csv and compose_trace.csv with a leading record_id column, and compose_records.csv, of a
    ``ComposedSequences`` whose composition is a ``Compositions`` (one group per record)."""
    comps = result.composition
    S, D = comps.n_states, comps.n_columns
    n_windows = np.bincount(result.owner, minlength=len(comps))
    with open(os.path.join(directory, "compose_profiles.csv"), 'w') as f:
        f.write("record_id,state,occupancy,self_transition,mean_region," + ("phage_score," if phage_score is not None else "")
                + ",".join("p%d" % j for j in range(D)) + "\n")
        for g, comp in enumerate(comps):
            if comp is None:
                continue
            for s in range(S):
                stay = float(comp.trans[s, s])
                f.write("%s,%d,%r,%r,%r,%s%s\n" % (result.record_ids[g], s, float(comp.occupancy[s]), stay,
                                                   result.step / (1.0 - stay),
                                                   ("%r," % float(phage_score[g][s])) if phage_score is not None else "",
                                                   ",".join(repr(float(v)) for v in np.exp(comp.log_profiles[s]))))
    with open(os.path.join(directory, "compose_trace.csv"), 'w') as f:
        f.write("record_id,iteration," + ",".join(TRACE_COLUMNS) + "\n")
        for g, trace in enumerate(comps.traces):
            for i, (L, F) in enumerate(trace):
                f.write("%s,%d,%r,%r\n" % (result.record_ids[g], i, float(L), float(F)))
    with open(os.path.join(directory, "compose_records.csv"), 'w') as f:
        f.write("record_id,n_windows,status,n_iter,converged,log_evidence,bic\n")
        for g in range(len(comps)):
            f.write("%s,%d,%d,%d,%d,%r,%r\n" % (result.record_ids[g], int(n_windows[g]), int(comps.status[g]),
                                                int(comps.n_iter[g]), int(comps.converged[g]), float(result.log_evidence[g]),
                                                float(comps.bic[g])))


def write_refined_files(directory, result):
    """compose_boundaries.csv (one line per refined boundary; gain and evidences in nats) and compose_segments_refined.csv
    (compose_segments.csv's columns, of ``refined_regions``) of a ``ComposedSequences`` whose ``refine`` has run."""
    os.makedirs(directory, exist_ok=True)
    b = result.boundaries
    if b is None:
        raise ValueError("write_refined_files needs the boundaries: call refine(fasta_or_sequences) first")
    with open(os.path.join(directory, "compose_boundaries.csv"), 'w') as f:
        f.write("record_id,window_boundary,position,left_state,right_state,gain,left_evidence,right_evidence,support\n")
        for i in range(len(b.position)):
            f.write("%s,%d,%d,%d,%d,%r,%r,%r,%d\n" % (b.record_id[i], int(b.window_boundary[i]), int(b.position[i]),
                                                     int(b.left_state[i]), int(b.right_state[i]), float(b.gain[i]),
                                                     float(b.left_evidence[i]), float(b.right_evidence[i]), int(b.support[i])))
    with open(os.path.join(directory, "compose_segments_refined.csv"), 'w') as f:
        f.write("record_id,start,end,state,n_windows,mean_posterior\n")
        for rid, a, e, s, nw, mp in result.refined_regions():
            f.write("%s,%d,%d,%d,%d,%r\n" % (rid, a, e, s, nw, mp))


def write_confidence_file(directory, result):
    """compose_boundary_confidence.csv (one line per refined boundary: the support interval, whether the search interval cut
    it short, and the posterior's figures) of a ``ComposedSequences`` whose ``refine(confidence=...)`` has run."""
    os.makedirs(directory, exist_ok=True)
    b, c = result.boundaries, result.boundary_confidence
    if b is None or c is None:
        raise ValueError("write_confidence_file needs the confidence: call refine(fasta_or_sequences, confidence=True) first")
    with open(os.path.join(directory, "compose_boundary_confidence.csv"), 'w') as f:
        f.write("record_id,window_boundary,position,lower,upper,n_within,at_lo,at_hi,mass_within,mass_at_position,mean_offset,"
                "rms_distance\n")
        for i in range(len(b.position)):
            f.write("%s,%d,%d,%d,%d,%d,%d,%d,%r,%r,%r,%r\n" % (
                b.record_id[i], int(b.window_boundary[i]), int(b.position[i]), int(c.lower[i]), int(c.upper[i]), int(c.n_within[i]),
                int(c.at_lo[i]), int(c.at_hi[i]), float(c.mass_within[i]), float(c.mass_at_position[i]), float(c.mean_offset[i]),
                float(c.rms_distance[i])))


def write_files(directory, result, phage_score=None):
    """compose_windows.csv, compose_segments.csv, compose_profiles.csv and compose_trace.csv of a ``ComposedSequences``; for
    one fitted per record (``segment_sequences(per_record=True)``) the last two gain a leading record_id column and
    compose_records.csv is written beside them.  (The two files of ``--refine``: ``write_refined_files``.)"""
    os.makedirs(directory, exist_ok=True)
    comp = result.composition
    S, D = (comp.n_states, comp.n_columns) if isinstance(comp, Compositions) else comp.log_profiles.shape
    with open(os.path.join(directory, "compose_windows.csv"), 'w') as f:
        f.write("record_id,start,state," + ",".join("posterior%d" % s for s in range(S)) + "\n")
        for i in range(len(result)):
            f.write("%s,%d,%d,%s\n" % (result.record_ids[int(result.owner[i])], int(result.start[i]), int(result.state[i]),
                                       ",".join(repr(float(v)) for v in result.posterior[i])))
    with open(os.path.join(directory, "compose_segments.csv"), 'w') as f:
        f.write("record_id,start,end,state,n_windows,mean_posterior\n")
        for rid, a, b, s, nw, mp in result.regions():
            f.write("%s,%d,%d,%d,%d,%r\n" % (rid, a, b, s, nw, mp))
    if isinstance(comp, Compositions):
        return _write_record_files(directory, result, phage_score)
    with open(os.path.join(directory, "compose_profiles.csv"), 'w') as f:
        f.write("state,occupancy,self_transition,mean_region," + ("phage_score," if phage_score is not None else "")
                + ",".join("p%d" % j for j in range(D)) + "\n")
        for s in range(S):
            stay = float(comp.trans[s, s])
            f.write("%d,%r,%r,%r,%s%s\n" % (s, float(comp.occupancy[s]), stay, result.step / (1.0 - stay),
                                            ("%r," % float(phage_score[s])) if phage_score is not None else "",
                                            ",".join(repr(float(v)) for v in np.exp(comp.log_profiles[s]))))
    with open(os.path.join(directory, "compose_trace.csv"), 'w') as f:
        f.write("iteration," + ",".join(TRACE_COLUMNS) + "\n")
        for i, (L, F) in enumerate(comp.trace):
            f.write("%d,%r,%r\n" % (i, float(L), float(F)))


def main(argv=None):
    args = _parser().parse_args(argv)
    if (args.positive_features is None) != (args.negative_features is None):
        raise SystemExit("-pf and -nf go together")
    options = dict(mean_region=args.mean_region, block=args.block, max_iter=args.max_iter, tol=args.tol,
                   fit_transitions=not args.keep_transitions)
    if args.temper is not None:
        options["temper"] = args.temper
    if args.scan is not None and args.scan is not True and args.scan < 1:
        raise SystemExit("--scan takes a number of windows >= 1")
    if args.per_record and args.scan is not None:
        raise SystemExit("--per_record does not go with --scan")
    if args.refine is not None and args.refine is not True and args.refine < 0:
        raise SystemExit("--refine takes a span in bases >= 0")
    if args.confidence is not None and args.refine is None:
        raise SystemExit("--confidence goes with --refine")
    if args.confidence is not None and args.confidence is not True and not (np.isfinite(args.confidence) and args.confidence >= 0):
        raise SystemExit("--confidence takes a number of nats >= 0")
    result = segment_sequences(args.input_file, args.states, args.window, args.step, args.kmer_length, args.both_strands,
                               args.scan, args.per_record, **options)
    score = None
    if args.positive_features is not None:
        from . import fileIO
        pos = fileIO.read_feature_file(args.positive_features, normalize=False)[1]
        neg = fileIO.read_feature_file(args.negative_features, normalize=False)[1]
        score = result.composition.label(pos, neg)
    write_files(args.output_directory, result, score)
    if args.refine is not None:
        result.refine(args.input_file, None if args.refine is True else args.refine, args.confidence)
        write_refined_files(args.output_directory, result)
        if args.confidence is not None:
            write_confidence_file(args.output_directory, result)
    return result


if __name__ == '__main__':
    main()
