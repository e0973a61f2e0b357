"""
mixture.py -- mixtures of multinomials fitted to integer count rows by EM (this project's own).

``likelihood`` keeps one component per reference row with equal weight.  This module fits K weighted components to count
rows c_i (N, D), with the row's length inside the model -- count-aware clustering, and a class summarised by K profiles:

    S[i,k]  = sum_j c_i[j] log theta_k[j] + log pi_k
    l_i     = logsumexp_k S[i,k]                 r[i,k] = exp(S[i,k] - l_i)
    T[k,j]  = sum_i r[i,k] c_i[j]     N_k = sum_i r[i,k]     L = sum_i l_i          (E-step: device, mixture.hip)
    theta_k[j] = (T[k,j] + a) / (sum_j T[k,j] + D a)         pi_k = N_k / sum_k N_k  (M-step: ``m_step``, NumPy)
    F       = L + a sum_k sum_j log theta_k[j]               (the penalised evidence: what this EM raises)

The log table and log pi are NumPy's, made here and uploaded; an iteration is one table upload, one device call and
``m_step``; the N x K responsibilities stay on the device.  A component whose N_k reaches 0 has pi = 0, contributes nothing
from then on and keeps the pseudocount's uniform profile; it is reported in ``Mixture.dead``, not an error.  Components
keep their start order.

    m_step(T, Nk, pseudocount)                                   (log_profiles (K, D), weights (K,))
    fit(counts_or_batch, n_components, ...)                      a Mixture
    from_rows(counts, pseudocount)                               one equal-weight component per row (rows <= 256)
    score(query_counts, positive_mixture, negative_mixture)      l_+ - l_-, the compressed likelihood.score
    load(path)                                                   a Mixture saved with Mixture.save
    python -m phamers_amd.mixture -in FEATURES|FASTA -K n -out DIR

Many fits side by side (mixture_sweep.hip): the rows go up once with their row sets, every
(K, start, fold) cell advances one EM iteration per device call, and each cell is bit for bit what ``fit`` gives alone.

    sweep(counts_or_batch, n_components, folds, ...)             a MixtureSweep: every cell, held-out evidence and BIC per K
    cross_validate(positive_counts, negative_counts, n_components, folds, ...)
                                                                 held-out l_+ - l_- per K (compare.mixture_cells), AUC, accuracy
    python -m phamers_amd.mixture_grid                           the two as tables per K
"""
import collections
import os

import numpy as np

from . import _lib
from .likelihood import _count_rows, _pseudocount, log_table

MAX_COMPONENTS = _lib.MIX_MAX_COMPONENTS
TRACE_COLUMNS = ("L", "F", "smallest_weight", "dead")


def m_step(T, Nk, pseudocount):
    """(log_profiles (K, D), weights (K,)) from the expected counts T (K, D) and N_k (K,): theta = (T + a) / (sum_j T + D a)
    and pi = N_k / sum_k N_k, one NumPy operation per sign written, then ``np.log`` of theta.  N_k = 0 gives pi = 0 (and,
    its T row being 0, the uniform profile).  ValueError for a pseudocount that is not finite and > 0."""
    a = _pseudocount(pseudocount)
    T = np.asarray(T, dtype=np.float64)
    Nk = np.asarray(Nk, dtype=np.float64)
    if T.ndim != 2 or Nk.shape != (T.shape[0],):
        raise ValueError("T must be (K, D) and Nk (K,)")
    theta = (T + a) / (T.sum(axis=1, keepdims=True) + T.shape[1] * a)
    return np.log(theta), Nk / Nk.sum()


def log_weights(weights):
    """np.log of the weights, -inf for a weight of 0 (no warning)."""
    with np.errstate(divide='ignore'):
        return np.log(np.asarray(weights, dtype=np.float64))


def evidence(L, log_profiles, pseudocount):
    """F = L + a sum_k sum_j log theta_k[j]."""
    return float(L) + float(pseudocount) * float(np.sum(log_profiles))


class _DeviceEStep(object):
    """The device half of a fit or of a Mixture's queries: the rows resident once, one table updated per call."""

    def __init__(self, counts_or_batch, batch_rows=0):
        self.ctx = _lib.get_context()
        self.own = not isinstance(counts_or_batch, _lib.Batch)
        self.host = None
        if self.own:
            self.host = _count_rows(counts_or_batch, "counts")
            self.batch = _lib.Batch.from_counts(self.ctx, self.host) if len(self.host) else None
        else:
            self.batch = counts_or_batch
        self.n = len(self.host) if self.host is not None else self.batch.n
        self.D = self.host.shape[1] if self.host is not None else self.batch.D
        self.batch_rows, self.table = batch_rows, None

    def rows(self, index):
        """uint32 count rows ``index`` of the data (the start rule)."""
        if self.host is not None:
            return self.host[index]
        sel = self.batch.select(np.asarray(index, dtype=np.uint64))
        try:
            return sel.counts_u32()
        finally:
            sel.close()

    def _table(self, log_profiles, log_w):
        if self.table is None or (self.table.K, self.table.D) != np.shape(log_profiles):
            if self.table is not None:
                self.table.close()
            self.table = _lib.MixtureTable(self.ctx, log_profiles, log_w)
        else:
            self.table.update(log_profiles, log_w)
        return self.table

    def __call__(self, log_profiles, log_w, rows=False):
        table = self._table(log_profiles, log_w)
        if self.batch is not None:
            return self.batch.mixture_expect(table, self.batch_rows, rows)
        return table.expect(self.host, self.batch_rows, rows)      # (rows a batch cannot hold: host counts every call)

    def responsibilities(self, log_profiles, log_w):
        table = self._table(log_profiles, log_w)
        if self.batch is not None:
            return self.batch.mixture_responsibilities(table, self.batch_rows)
        return table.responsibilities(self.host, self.batch_rows)

    def close(self):
        if self.table is not None:
            self.table.close()
        if self.own and self.batch is not None:
            self.batch.close()


def _estep(counts_or_batch, batch_rows=0):
    """The E-step object of ``counts_or_batch`` (the tests put the statement in its place)."""
    return _DeviceEStep(counts_or_batch, batch_rows)


def _components(n_components, n_rows=None):
    K = int(n_components)
    if not 1 <= K <= MAX_COMPONENTS:
        raise ValueError("n_components must be 1 to %d, got %r" % (MAX_COMPONENTS, n_components))
    if n_rows is not None and K > n_rows:
        raise ValueError("n_components = %d exceeds the %d rows" % (K, n_rows))
    return K


def start(estep, n_components, pseudocount, init=None, seed=None):
    """(log_profiles (K, D), weights (K,)) a fit starts from.  ``init``: K row indices (the rows' smoothed profiles), a
    (K, D) array of profiles (positive, normalised here), or None = np.random.RandomState(seed).choice(N, K, replace=False).
    The weights are uniform."""
    K = _components(n_components, estep.n)
    init = None if init is None else np.asarray(init)
    if init is not None and init.ndim == 2:
        p = np.asarray(init, dtype=np.float64)
        if p.shape != (K, estep.D) or not (np.isfinite(p).all() and (p > 0).all()):
            raise ValueError("init profiles must be (%d, %d), finite and > 0" % (K, estep.D))
        logp = np.log(p / p.sum(axis=1, keepdims=True))
    else:
        index = np.random.RandomState(seed).choice(estep.n, K, replace=False) if init is None else init
        index = np.asarray(index)
        if index.shape != (K,) or not np.issubdtype(index.dtype, np.integer) or index.min() < 0 or index.max() >= estep.n:
            raise ValueError("init must be %d row indices below %d, or (K, D) profiles" % (K, estep.n))
        logp = log_table(estep.rows(index), pseudocount)
    return logp, np.full(K, 1.0 / K)


Fitted = collections.namedtuple("Fitted", "log_profiles weights trace n_iter converged T")


def _em(estep, logp, w, pseudocount, max_iter, tol):
    """EM from (logp, w): at most ``max_iter`` M-steps, every iterate's evidence in the trace; the loop stops at the
    first iterate with F_i - F_{i-1} <= tol max(1, |F_i|), which is returned -- the trace's last row is its evidence."""
    trace, F_prev, converged = [], None, False
    for it in range(max_iter + 1):
        T, Nk, L = estep(logp, log_weights(w))[:3]
        F = evidence(L, logp, pseudocount)
        trace.append((L, F, float(w.min()), int((w == 0).sum())))
        if F_prev is not None and F - F_prev <= tol * max(1.0, abs(F)):
            converged = True
            break
        if it == max_iter:
            break
        F_prev = F
        logp, w = m_step(T, Nk, pseudocount)
    return Fitted(logp, w, np.array(trace, dtype=np.float64).reshape(-1, len(TRACE_COLUMNS)), len(trace) - 1, converged, T)


class Mixture(object):
    """A fitted mixture: ``log_profiles`` (K, D), ``weights`` (K,), ``pseudocount``, ``n_iter`` (M-steps), ``converged``,
    ``dead`` (K,) bool: the components of weight 0, ``trace`` (iterates, 4): L, F, smallest weight, dead components, and
    ``effective_kmers`` (K,): sum_j T[k, j] of the last E-step."""

    def __init__(self, log_profiles, weights, pseudocount, n_iter=0, converged=False, trace=None, effective_kmers=None):
        self.log_profiles = np.ascontiguousarray(log_profiles, dtype=np.float64)
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        if self.log_profiles.ndim != 2 or self.weights.shape != (self.log_profiles.shape[0],):
            raise ValueError("log_profiles must be (K, D) and weights (K,)")
        _components(self.log_profiles.shape[0])
        self.pseudocount, self.n_iter, self.converged = float(pseudocount), int(n_iter), bool(converged)
        self.trace = np.zeros((0, len(TRACE_COLUMNS))) if trace is None else np.asarray(trace, dtype=np.float64)
        self.effective_kmers = (np.full(len(self.weights), np.nan) if effective_kmers is None
                                else np.asarray(effective_kmers, dtype=np.float64))

    @property
    def dead(self):
        return self.weights == 0

    @property
    def n_components(self):
        return len(self.weights)

    def _on(self, counts, call):
        estep = _estep(counts)
        try:
            if estep.D != self.log_profiles.shape[1]:
                raise ValueError("the counts have %d columns, the mixture %d" % (estep.D, self.log_profiles.shape[1]))
            return call(estep)
        finally:
            estep.close()

    def expect(self, counts):
        """(T (K, D), N_k (K,), L) of one E-step over ``counts`` (count rows or a resident batch)."""
        return self._on(counts, lambda e: e(self.log_profiles, log_weights(self.weights))[:3])

    def log_likelihood(self, counts):
        """l_i (N,) float64: the log-likelihood of every row under the mixture (without the multinomial coefficient)."""
        return self._on(counts, lambda e: e(self.log_profiles, log_weights(self.weights), rows=True)[3])

    def responsibilities(self, counts):
        """r (N, K) float64: the one call that brings the N x K matrix to the host."""
        return self._on(counts, lambda e: e.responsibilities(self.log_profiles, log_weights(self.weights))[0])

    def assign(self, counts):
        """(component (N,) int64, responsibility (N,)): the argmax of r per row, lowest index on ties, found on the device."""
        out = self._on(counts, lambda e: e(self.log_profiles, log_weights(self.weights), rows=True))
        return out[4].astype(np.int64), out[5]

    def save(self, path):
        """A ``.npz`` file that ``load`` reads back."""
        with open(path, 'wb') as f:
            np.savez(f, log_profiles=self.log_profiles, weights=self.weights, pseudocount=self.pseudocount,
                     n_iter=self.n_iter, converged=self.converged, trace=self.trace, effective_kmers=self.effective_kmers)


def load(path):
    """The Mixture of a file written by ``Mixture.save``."""
    with np.load(path) as z:
        return Mixture(z["log_profiles"], z["weights"], float(z["pseudocount"]), int(z["n_iter"]), bool(z["converged"]),
                       z["trace"], z["effective_kmers"])


def fit(counts_or_batch, n_components, pseudocount=0.5, init=None, seed=None, n_init=1, max_iter=100, tol=1e-6,
        _batch_rows=0):
    """A K-component mixture of multinomials fitted by EM to the count rows ``counts_or_batch``: an integer matrix (N, D)
    (made resident once) or a ``_lib.Batch`` (used where it lies).  ``init``: see ``start``.  The loop stops when
    F_i - F_{i-1} <= tol max(1, |F_i|) or after ``max_iter`` M-steps.  ``n_init`` > 1 runs the seeds seed, seed + 1, ... one
    after another and keeps the largest F (the lowest seed on ties).  ValueError for frequencies, K outside 1..256, K > N,
    a pseudocount that is not finite and > 0.  ``_batch_rows`` (rows per device batch) is for the tests: no result depends
    on it."""
    a = _pseudocount(pseudocount)
    _components(n_components)
    n_init, max_iter, tol = int(n_init), int(max_iter), float(tol)
    if n_init < 1 or max_iter < 0 or not (np.isfinite(tol) and tol >= 0):
        raise ValueError("n_init >= 1, max_iter >= 0 and a finite tol >= 0 are required")
    if n_init > 1 and init is not None:
        raise ValueError("n_init > 1 needs seeded starts: init must be None")
    estep = _estep(counts_or_batch, _batch_rows)
    try:
        best = None
        for i in range(n_init):
            logp, w = start(estep, n_components, a, init, None if seed is None else int(seed) + i)
            got = _em(estep, logp, w, a, max_iter, tol)
            if best is None or got.trace[-1, 1] > best.trace[-1, 1]:
                best = got
    finally:
        estep.close()
    return Mixture(best.log_profiles, best.weights, a, best.n_iter, best.converged, best.trace, best.T.sum(axis=1))


def from_rows(counts, pseudocount=0.5):
    """The mixture ``likelihood`` scores with: one component per count row of ``counts`` (M <= 256, D), equal weights."""
    logp = log_table(counts, pseudocount)
    K = _components(logp.shape[0])
    return Mixture(logp, np.full(K, 1.0 / K), pseudocount)


def score(query_counts, positive_mixture, negative_mixture, per_kmer=False):
    """l_+(q) - l_-(q) in nats for every count row of ``query_counts`` (N, D) under two mixtures: (N,) float64, the
    compressed counterpart of likelihood.score.  ``per_kmer``: divided by the row's total."""
    from .likelihood import _per_kmer
    q = _count_rows(query_counts, "query_counts")
    s = positive_mixture.log_likelihood(q) - negative_mixture.log_likelihood(q)
    return _per_kmer(s, q) if per_kmer else s


# ---- many fits side by side ------------------------------------------------------------------------
def _sweep_device(counts_or_batch, row_sets):
    """The device half of a sweep: the rows and their row sets resident, ``step(jobs, rows, _budget_bytes, expect)`` and
    ``close()`` (the tests put the statement in its place)."""
    return _lib.MixtureSweep(_lib.get_context(), counts_or_batch, row_sets)


def _evaluate(positive_scores, negative_scores):
    """(ROC area, accuracy at threshold 0) of a scoring, on the device (the tests put NumPy in its place)."""
    from .likelihood import evaluate
    return evaluate(positive_scores, negative_scores)


class _SetRows(object):
    """What ``start`` asks of an E-step object, for one row set of host counts."""

    def __init__(self, host, index):
        self.host, self.index, self.n, self.D = host, index, len(index), host.shape[1]

    def rows(self, index):
        return self.host[self.index[index]]


def _host_rows(counts_or_batch):
    if isinstance(counts_or_batch, _lib.Batch):
        return counts_or_batch.counts_u32()
    return _count_rows(counts_or_batch, "counts")


def _sweep_arguments(n_components, n_init, max_iter, tol, pseudocount):
    a = _pseudocount(pseudocount)
    Ks = [_components(K) for K in np.atleast_1d(np.asarray(n_components)).tolist()]
    if not Ks or len(set(Ks)) != len(Ks):
        raise ValueError("n_components must be a list of distinct component counts")
    n_init, max_iter, tol = int(n_init), int(max_iter), float(tol)
    if n_init < 1 or max_iter < 0 or not (np.isfinite(tol) and tol >= 0):
        raise ValueError("n_init >= 1, max_iter >= 0 and a finite tol >= 0 are required")
    return a, Ks, n_init, max_iter, tol


def _lockstep(dev, host, sets, cells, a, max_iter, tol):
    """``_em`` for every cell (row set, K, seed) at once: one ``dev.step`` over the cells still running per iteration, then
    ``m_step`` and ``_em``'s stopping rule per cell; a cell that stops leaves the job list.  A list of ``Fitted`` whose T
    is sum_j T[k, j]."""
    state = []
    for s, K, seed in cells:
        logp, w = start(_SetRows(host, sets[s]), K, a, None, seed)
        state.append(dict(set=s, logp=logp, w=w, trace=[], F_prev=None, done=None))
    running = list(range(len(cells)))
    for it in range(max_iter + 1):
        if not running:
            break
        out = dev.step([(state[c]["set"], state[c]["logp"], log_weights(state[c]["w"])) for c in running])
        still = []
        for c, (T, Nk, L, _) in zip(running, out):
            st = state[c]
            F = evidence(L, st["logp"], a)
            st["trace"].append((L, F, float(st["w"].min()), int((st["w"] == 0).sum())))
            converged = st["F_prev"] is not None and F - st["F_prev"] <= tol * max(1.0, abs(F))
            if converged or it == max_iter:
                trace = np.array(st["trace"], dtype=np.float64).reshape(-1, len(TRACE_COLUMNS))
                st["done"] = Fitted(st["logp"], st["w"], trace, len(trace) - 1, bool(converged), T.sum(axis=1))
                continue
            st["F_prev"] = F
            st["logp"], st["w"] = m_step(T, Nk, a)
            still.append(c)
        running = still
    return [st["done"] for st in state]


def _best_start(fits):
    """The index of the largest final evidence F, the lowest on ties (``fit``'s rule)."""
    best = 0
    for i in range(1, len(fits)):
        if fits[i].trace[-1, 1] > fits[best].trace[-1, 1]:
            best = i
    return best


def _as_mixture(fitted, a):
    return Mixture(fitted.log_profiles, fitted.weights, a, fitted.n_iter, fitted.converged, fitted.trace, fitted.T)


def _bic(fitted, n_rows):
    """-2 L + (live (D - 1) + live - 1) ln N of a fit on ``n_rows`` rows; live: the components that are not dead."""
    live = int((fitted.weights != 0).sum())
    return -2.0 * float(fitted.trace[-1, 0]) + (live * (fitted.log_profiles.shape[1] - 1) + live - 1) * float(np.log(n_rows))


class MixtureSweep(object):
    """What ``sweep`` returns.  ``n_components`` (the K values), ``n_init``, ``n_folds``, ``fold_of`` (N,); over (K, init,
    fold) with the all-rows fit as the last fold: ``F``, ``L`` (final evidence and log-likelihood of the training rows),
    ``n_iter``, ``converged``, ``dead`` (components of weight 0); ``held_out_log_likelihood`` (K, N), NaN where a row is
    never held out; ``held_out_per_kmer`` (K,): sum l_i / sum k-mers over the held-out rows; ``bic`` (K,)."""

    def __init__(self, Ks, n_init, n_folds, fold_of, fits, pseudocount):
        self.n_components, self.n_init, self.n_folds, self.fold_of = list(Ks), n_init, n_folds, fold_of
        self.pseudocount, self._fits = pseudocount, fits            # fits[a][i][f]: a Fitted
        shape = (len(Ks), n_init, n_folds + 1)
        cell = lambda get, dtype: np.array([[[get(fits[a][i][f]) for f in range(shape[2])] for i in range(shape[1])]
                                            for a in range(shape[0])], dtype=dtype).reshape(shape)
        self.F, self.L = cell(lambda g: g.trace[-1, 1], np.float64), cell(lambda g: g.trace[-1, 0], np.float64)
        self.n_iter, self.converged = cell(lambda g: g.n_iter, np.int64), cell(lambda g: g.converged, bool)
        self.dead = cell(lambda g: int((g.weights == 0).sum()), np.int64)

    def _k(self, K):
        if int(K) not in self.n_components:
            raise ValueError("K = %r is not one of %r" % (K, self.n_components))
        return self.n_components.index(int(K))

    def _fold(self, fold):
        if fold is not None and not 0 <= int(fold) < self.n_folds:
            raise ValueError("fold must be 0 to %d, or None" % (self.n_folds - 1))
        return self.n_folds if fold is None else int(fold)

    def best_init(self, K, fold=None):
        """The start ``mixture(K, None, fold)`` returns: the largest training F, the lowest seed on ties."""
        f = self._fold(fold)
        return _best_start([self._fits[self._k(K)][i][f] for i in range(self.n_init)])

    def mixture(self, K, init=None, fold=None):
        """The ``Mixture`` of cell (K, init, fold): ``init=None`` the best start, ``fold=None`` the fit on all rows."""
        f = self._fold(fold)
        i = self.best_init(K, fold) if init is None else int(init)
        if not 0 <= i < self.n_init:
            raise ValueError("init must be 0 to %d, or None" % (self.n_init - 1))
        return _as_mixture(self._fits[self._k(K)][i][f], self.pseudocount)

    def best(self, criterion='held_out'):
        """The K of the largest held-out evidence per k-mer, or of the smallest BIC (the first such K on a tie)."""
        if criterion == 'held_out':
            if self.n_folds == 0:
                raise ValueError("held-out evidence needs folds")
            return self.n_components[int(np.argmax(self.held_out_per_kmer))]
        if criterion == 'bic':
            return self.n_components[int(np.argmin(self.bic))]
        raise ValueError("criterion must be 'held_out' or 'bic'")

    def table(self):
        """One dict per K: K, held_out_per_kmer, bic, mean_iterations (over every cell of the K), dead (components of weight
        0 in the all-rows best start)."""
        return [dict(K=K, held_out_per_kmer=float(self.held_out_per_kmer[a]), bic=float(self.bic[a]),
                     mean_iterations=float(self.n_iter[a].mean()), dead=int(self.dead[a, self.best_init(K), self.n_folds]))
                for a, K in enumerate(self.n_components)]


def _fold_sets(fold_of, n_folds, offset=0):
    """(training rows, held-out rows) per fold, as ascending row indices shifted by ``offset``."""
    return ([offset + np.flatnonzero(fold_of != f) for f in range(n_folds)],
            [offset + np.flatnonzero(fold_of == f) for f in range(n_folds)])


def _check_training(Ks, sets):
    smallest = min(len(s) for s in sets)
    if max(Ks) > smallest:
        raise ValueError("n_components = %d exceeds the %d rows of the smallest training set" % (max(Ks), smallest))


def sweep(counts_or_batch, n_components, folds=0, fold_seed=None, seed=0, n_init=1, pseudocount=0.5, max_iter=100, tol=1e-6,
          groups=None):
    """Every cell (K, start i, fold f) of a grid fitted in lock step: cell (K, i, f) is ``fit(rows outside fold f, K,
    seed=seed + i, ...)`` field by field, and every K also has the fit on all rows.  The fold of row i is ``groups[i]`` (an
    integer >= 0, or -1 for a row that is never held out), else cross_validate.FoldPlan(N, 0, folds, fold_seed).positive;
    ``folds=0`` without ``groups``: no folds.  One device call per EM iteration over the cells still running, one more for
    the held-out rows under every fold's best start.  A ``MixtureSweep``.  ValueError for K outside 1..256 or above the
    smallest training set, ``folds`` of 1 or above N, frequencies, and what ``fit`` refuses."""
    a, Ks, n_init, max_iter, tol = _sweep_arguments(n_components, n_init, max_iter, tol, pseudocount)
    host = _host_rows(counts_or_batch)
    N = len(host)
    if groups is not None:
        fold_of = np.asarray(groups)
        if fold_of.shape != (N,) or not np.issubdtype(fold_of.dtype, np.integer) or fold_of.min() < -1:
            raise ValueError("groups: one integer >= -1 per row (%d)" % N)
        fold_of = fold_of.astype(np.int64)
        n_folds = int(fold_of.max()) + 1
        if n_folds and np.bincount(fold_of[fold_of >= 0], minlength=n_folds).min() == 0:
            raise ValueError("groups: every fold 0 .. %d needs a row" % (n_folds - 1))
    else:
        n_folds = int(folds)
        if n_folds == 1 or n_folds < 0 or n_folds > N:
            raise ValueError("folds must be 0 or 2 to the %d rows, got %r" % (N, folds))
        from .cross_validate import FoldPlan
        fold_of = FoldPlan(N, 0, n_folds, fold_seed).positive.astype(np.int64) if n_folds else np.full(N, -1, dtype=np.int64)
    if N == 0:
        raise ValueError("n_components = %d exceeds the 0 rows" % max(Ks))
    train, held = _fold_sets(fold_of, n_folds)
    sets = train + [np.arange(N)] + held               # set f: fold f's training rows; n_folds: all rows; then the held-out rows
    _check_training(Ks, sets[:n_folds + 1])
    cells = [(f, K, int(seed) + i) for K in Ks for i in range(n_init) for f in range(n_folds + 1)]
    dev = _sweep_device(counts_or_batch if isinstance(counts_or_batch, _lib.Batch) else host, sets)
    try:
        done = _lockstep(dev, host, sets, cells, a, max_iter, tol)
        fits = [[[done[(b * n_init + i) * (n_folds + 1) + f] for f in range(n_folds + 1)] for i in range(n_init)]
                for b in range(len(Ks))]
        out = MixtureSweep(Ks, n_init, n_folds, fold_of, fits, a)
        out.held_out_log_likelihood = np.full((len(Ks), N), np.nan)
        jobs, where = [], []
        for b, K in enumerate(Ks):
            for f in range(n_folds):
                g = fits[b][out.best_init(K, f)][f]
                jobs.append((n_folds + 1 + f, g.log_profiles, log_weights(g.weights)))
                where.append((b, held[f]))
        for (b, index), got in zip(where, dev.step(jobs, rows=True, expect=False) if jobs else []):
            out.held_out_log_likelihood[b, index] = got[3]
    finally:
        dev.close()
    kmers = float(host[fold_of >= 0].sum(dtype=np.uint64))
    out.held_out_per_kmer = np.nansum(out.held_out_log_likelihood, axis=1) / kmers if n_folds else np.full(len(Ks), np.nan)
    out.bic = np.array([_bic(fits[b][out.best_init(K)][n_folds], N) for b, K in enumerate(Ks)])
    return out


CrossValidated = collections.namedtuple(
    "CrossValidated", "n_components n_pos scores auc accuracy held_out_per_kmer_positive held_out_per_kmer_negative "
                      "bic_positive bic_negative mean_iterations dead")


def cross_validate(positive_counts, negative_counts, n_components, folds, seed=None, fit_seed=0, n_init=1, pseudocount=0.5,
                   max_iter=100, tol=1e-6, bic=False):
    """Held-out scores l_+ - l_- of every row per K, under the two mixtures fitted to its fold's training rows: the split
    is cross_validate.FoldPlan(n_pos, n_neg, folds, seed), both classes' training sets and the joint held-out sets are row
    sets of one sweep object over vstack(positive, negative), and all 2 folds len(Ks) n_init fits run in lock step (start
    i of a fit has seed fit_seed + i; the best start is ``fit``'s).  Row K of ``scores`` (len(Ks), n_pos + n_neg),
    positives first, equals the loop of ``fit`` on each fold's training rows and ``score`` on its held-out rows.  A
    ``CrossValidated``: also ``auc`` and ``accuracy`` at 0 per K, the held-out evidence per k-mer of each class under its
    own mixtures, ``mean_iterations`` and ``dead`` (components of weight 0, summed over the folds' best starts); ``bic``:
    also fit each whole class per K for ``bic_positive`` / ``bic_negative`` (NaN otherwise)."""
    a, Ks, n_init, max_iter, tol = _sweep_arguments(n_components, n_init, max_iter, tol, pseudocount)
    pos, neg = _count_rows(positive_counts, "positive_counts"), _count_rows(negative_counts, "negative_counts")
    if pos.ndim != 2 or neg.ndim != 2 or pos.shape[1] != neg.shape[1]:
        raise ValueError("the two classes must have the same number of columns")
    n_pos, n_neg, n_folds = len(pos), len(neg), int(folds)
    if n_folds < 2 or n_folds > min(n_pos, n_neg):
        raise ValueError("folds must be 2 to the rows of the smaller class (%d), got %r" % (min(n_pos, n_neg), folds))
    from .cross_validate import FoldPlan
    plan = FoldPlan(n_pos, n_neg, n_folds, seed)
    host = np.vstack((pos, neg))
    train_p, held_p = _fold_sets(plan.positive, n_folds)
    train_n, held_n = _fold_sets(plan.negative, n_folds, n_pos)
    whole = [np.arange(n_pos), n_pos + np.arange(n_neg)] if bic else []
    held = [np.concatenate((hp, hn)) for hp, hn in zip(held_p, held_n)]
    sets = train_p + train_n + held + whole      # set f / n_folds + f: the classes' training rows; 2 n_folds + f: held out
    _check_training(Ks, train_p + train_n)
    fitted_sets = list(range(2 * n_folds)) + [3 * n_folds + c for c in range(len(whole))]
    cells = [(s, K, int(fit_seed) + i) for K in Ks for s in fitted_sets for i in range(n_init)]
    dev = _sweep_device(host, sets)
    try:
        done = _lockstep(dev, host, sets, cells, a, max_iter, tol)
        best, at = {}, 0
        for K in Ks:
            for s in fitted_sets:
                best[K, s] = done[at + _best_start(done[at:at + n_init])]
                at += n_init
        jobs = [(2 * n_folds + f, best[K, c * n_folds + f].log_profiles, log_weights(best[K, c * n_folds + f].weights))
                for K in Ks for f in range(n_folds) for c in (0, 1)]
        got = iter(dev.step(jobs, rows=True, expect=False))
        scores = np.full((len(Ks), n_pos + n_neg), np.nan)
        evidence_p, evidence_n = np.zeros(len(Ks)), np.zeros(len(Ks))
        for b, K in enumerate(Ks):
            for f in range(n_folds):
                lp, ln = next(got)[3], next(got)[3]
                scores[b, held[f]] = lp - ln
                evidence_p[b] += lp[:len(held_p[f])].sum()
                evidence_n[b] += ln[len(held_p[f]):].sum()
    finally:
        dev.close()
    ev = [_evaluate(s[:n_pos], s[n_pos:]) for s in scores]
    per_K = len(fitted_sets) * n_init
    nan = np.full(len(Ks), np.nan)
    return CrossValidated(
        Ks, n_pos, scores, np.array([e[0] for e in ev], dtype=np.float64), np.array([e[1] for e in ev], dtype=np.float64),
        evidence_p / float(pos.sum(dtype=np.uint64)), evidence_n / float(neg.sum(dtype=np.uint64)),
        np.array([_bic(best[K, 3 * n_folds], n_pos) for K in Ks]) if bic else nan,
        np.array([_bic(best[K, 3 * n_folds + 1], n_neg) for K in Ks]) if bic else nan,
        np.array([np.mean([g.n_iter for g in done[b * per_K:(b + 1) * per_K]]) for b in range(len(Ks))]),
        np.array([sum(int((best[K, s].weights == 0).sum()) for s in range(2 * n_folds)) for K in Ks], dtype=np.int64))


# ---- command line ---------------------------------------------------------------------------------------------------------
def _parser():
    import argparse
    ap = argparse.ArgumentParser(description="Fit a mixture of multinomials to the k-mer count rows of a file",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument('-in', '--input_file', required=True, help="Features (count) file, or FASTA file to count")
    ap.add_argument('-K', '--components', type=int, required=True, help="Components of the mixture (1 to 256)")
    ap.add_argument('-k', '--kmer_length', type=int, default=4, help="k-mer length when the input is a FASTA file")
    ap.add_argument('--seed', type=int, default=None, help="Seed of the start rows")
    ap.add_argument('--n_init', type=int, default=1, help="Seeded starts; the largest evidence is kept")
    ap.add_argument('--max_iter', type=int, default=100, help="Most M-steps of a start")
    ap.add_argument('--tol', type=float, default=1e-6, help="Relative gain of the evidence below which EM stops")
    ap.add_argument('--pseudocount', type=float, default=0.5, help="Pseudocount of the profiles")
    ap.add_argument('-out', '--output_directory', required=True, help="Directory of the three CSV files")
    return ap


def _is_fasta(path):
    import gzip
    opener = gzip.open if path.endswith('.gz') else open
    with opener(path, 'rb') as f:
        return f.read(1) == b'>'


def write_files(directory, mix, ids, component, responsibility, row_ll, totals):
    """mixture_components.csv, mixture_assignments.csv and mixture_trace.csv of a fit in ``directory``."""
    os.makedirs(directory, exist_ok=True)
    D = mix.log_profiles.shape[1]
    with open(os.path.join(directory, "mixture_components.csv"), 'w') as f:
        f.write("component,weight,effective_kmers,dead," + ",".join("p%d" % j for j in range(D)) + "\n")
        for k in range(mix.n_components):
            f.write("%d,%r,%r,%d,%s\n" % (k, float(mix.weights[k]), float(mix.effective_kmers[k]), int(mix.dead[k]),
                                          ",".join(repr(float(v)) for v in np.exp(mix.log_profiles[k]))))
    with np.errstate(invalid='ignore', divide='ignore'):
        per_kmer = row_ll / np.asarray(totals, dtype=np.float64)
    with open(os.path.join(directory, "mixture_assignments.csv"), 'w') as f:
        f.write("id,component,responsibility,log_likelihood,log_likelihood_per_kmer\n")
        for i in range(len(component)):
            f.write("%s,%d,%r,%r,%r\n" % (ids[i], component[i], float(responsibility[i]), float(row_ll[i]), float(per_kmer[i])))
    with open(os.path.join(directory, "mixture_trace.csv"), 'w') as f:
        f.write("iteration," + ",".join(TRACE_COLUMNS) + "\n")
        for i, (L, F, wmin, dead) in enumerate(mix.trace):
            f.write("%d,%r,%r,%r,%d\n" % (i, float(L), float(F), float(wmin), int(dead)))


def main(argv=None):
    args = _parser().parse_args(argv)
    _pseudocount(args.pseudocount)
    _components(args.components)
    fasta = batch = None
    try:
        if _is_fasta(args.input_file):
            fasta = _lib.Fasta(args.input_file)
            ids = fasta.phamers_ids()
            data = batch = _lib.Batch.from_fasta(_lib.get_context(), fasta, args.kmer_length)
            totals = batch.row_sums().astype(np.float64)
        else:
            from . import fileIO
            ids, data = fileIO.read_feature_file(args.input_file, normalize=False)
            data = _count_rows(data, "the rows of %s" % args.input_file)
            totals = data.sum(axis=1, dtype=np.uint64).astype(np.float64)
        mix = fit(data, args.components, args.pseudocount, None, args.seed, args.n_init, args.max_iter, args.tol)
        estep = _estep(data)
        try:
            _, _, _, row_ll, component, responsibility = estep(mix.log_profiles, log_weights(mix.weights), rows=True)
        finally:
            estep.close()
    finally:
        if batch is not None:
            batch.close()
        if fasta is not None:
            fasta.close()
    write_files(args.output_directory, mix, ids, component, responsibility, row_ll, totals)
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
