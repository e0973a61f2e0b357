"""The statement of the S-state chain over window count rows (phamers_amd/compose.py, csrc/chain.hip)
that the host and GPU tests compare against, and the bounds derived for the device's arithmetic.

Model.  Records r with windows t = offsets[r] .. offsets[r + 1] - 1, count rows c_t[D], S states with log profiles
log theta_s[D] (float64, as uploaded), transition A, start pi, temper:

    E[t][s] = temper * sum_j c_t[j] log theta_s[j]                    (``exact_emissions``: longdouble)
    d[t][s] = float64(E[t][s] - max_s' E[t][s'])                      (one IEEE subtraction: part of the model)
    e[t][s] = exp(d[t][s])

(i)   ``viterbi``: Python-int max-plus over q[t][s] = rint(max(d, -2^15) 2^16), ties to the smallest predecessor, a tie
      at the end to the smallest state.  The device must give this path and score bit for bit on its own E.
(ii)  ``forward_backward``: sequential longdouble, alpha normalised by each step's own sum; gamma, xi, gamma_0, the log
      evidence; ``expect`` adds T = gamma^T C and N_s over the records.
(iii) ``brute_force``: all S^n paths (n <= 7, S <= 3) in longdouble and Python ints.

Bounds (u = 2^-53).

Emissions.  The device sums the D products of a row on the matrix pipe in the tile's order (gram_tile.h: 8 columns per
k-slot and K step, four k-slots per instruction, K steps in column order).  Whatever the order, a term passes through at
most D - 1 additions, each rounding once; a product rounds at most once (not at all where fused); the multiply by temper
rounds once; the longdouble statement's own error and the second-order terms stay below one more u.  So

    |E - exact| <= (D + EMISSION_C) u temper sum_j c_j |log theta_j|,          EMISSION_C = 3

Forward-backward.  Every quantity is a sum of products of positive numbers.  A forward step costs, per state, S products
alpha_i A_ij and S - 1 additions (1 u each, a fused pair counts once), one product with e, and e itself errs by
EXP_ULP ulp <= 2 EXP_ULP u relative (tests/segment_ref.py: measured on the device once); rescaling by a power of two is
exact.  So alpha_t carries at most t (2 S + 2 EXP_ULP) u, beta_t (n - t) (2 S + 2 EXP_ULP) u, and a step's S^2 terms
alpha_{t-1}(i) A_ij e_t(j) beta_t(j) carry their sum plus 3 products; column sum, total, reciprocal and product add
2 S + 2.  Numerator and denominator of the quotient each carry that, hence

    |gamma - exact| <= B(n, S) exact + FLOOR,        B(n, S) = 2 (n (2 S + 1 + 2 EXP_ULP) + 4 S + 8) u

FLOOR = 2^-1000 is the format's: exp(d) below 2^-1022 is subnormal or 0 ("certain").  xi of a record adds one rounding per
step: (B + n u) exact + n FLOOR.  T and N_s are sums of n_rows positive terms gamma c in some fixed order (blocks of 1024
rows on the matrix pipe, then the 256-row tree): (B + (n_rows + 2) u) exact + FLOOR sum c.  Sums over R records add
R u more.  The log evidence is log(m) + (exponent) ln 2 + sum_t max_s E[t][s]: alpha's relative error is absolute on
the logarithm, the last sum of S terms adds S u, the sum of the n maxima n u sum|M|, the four final operations 8 u of
the magnitudes:

    |log_evidence - exact| <= (n (2 S + 1 + 2 EXP_ULP) + 4 S + 8) u + n u sum|M| + 8 u (|log_evidence| + sum|M| + 1)
"""
import itertools

import numpy as np

from tests.segment_ref import CLAMP, EXP_ULP, FLOOR, LD, QUANT_BITS, U

EMISSION_C = 3.0


# ---- emissions ---------------------------------------------------------------------------------------------------------------
def exact_emissions(counts, log_profiles, temper=1.0):
    """E (n, S) longdouble: counts as integers times the float64 logarithms, summed in longdouble, times temper."""
    c = np.asarray(counts).astype(LD)
    lp = np.asarray(log_profiles, dtype=np.float64).astype(LD)
    return LD(temper) * np.array([[np.sum(row * p) for p in lp] for row in c], dtype=LD).reshape(len(c), len(lp))


def emission_bound(counts, log_profiles, temper=1.0):
    """(n, S) float64: (D + EMISSION_C) u temper sum_j c_j |log theta_j|."""
    c = np.asarray(counts).astype(np.float64)
    mag = c @ np.abs(np.asarray(log_profiles, dtype=np.float64)).T
    return (c.shape[1] + EMISSION_C) * U * float(temper) * mag * (1.0 + 2.0 ** -40)


def relative(E):
    """d (n, S) float64 = E - max_s E, one IEEE subtraction."""
    E = np.asarray(E, dtype=np.float64)
    return E - E.max(axis=1, keepdims=True) if E.size else E.copy()


def quantise(E):
    """q[t][s] = rint(max(d, -2^15) 2^16) as Python ints (a list of lists)."""
    d = relative(E)
    return [[int(v) for v in row] for row in np.rint(np.maximum(d, -CLAMP) * 2.0 ** QUANT_BITS)]


def quantise_log(p):
    """The caller's quantised logarithms (segment.quantise) as Python ints, shaped as ``p``."""
    return np.rint(np.clip(np.log(np.asarray(p, dtype=np.float64)), -CLAMP, CLAMP) * 2.0 ** QUANT_BITS).astype(np.int64)


# ---- (i) -----------------------------------------------------------------------------------------------------------------
def viterbi(q, qlog_trans, qlog_init):
    """(states (n,) uint8, score int) of one record's integer emissions ``q`` (n lists of S Python ints)."""
    n = len(q)
    if n == 0:
        return np.zeros(0, dtype=np.uint8), 0
    S = len(q[0])
    qa = [[int(qlog_trans[i][j]) for j in range(S)] for i in range(S)]
    d = [int(qlog_init[j]) + q[0][j] for j in range(S)]
    back = []
    for t in range(1, n):
        nd, bp = [], []
        for j in range(S):
            best, k = d[0] + qa[0][j], 0
            for i in range(1, S):
                c = d[i] + qa[i][j]
                if c > best:
                    best, k = c, i
            nd.append(best + q[t][j])
            bp.append(k)
        d = nd
        back.append(bp)
    s = 0
    for j in range(1, S):
        if d[j] > d[s]:
            s = j
    score = d[s]
    states = np.empty(n, dtype=np.uint8)
    states[n - 1] = s
    for t in range(n - 1, 0, -1):
        s = back[t - 1][s]
        states[t - 1] = s
    return states, score


def viterbi_records(E, offsets, qlog_trans, qlog_init):
    """(states (n,), scores [R] Python ints) over every record of the float64 emissions ``E``."""
    q = quantise(E)
    off = [int(o) for o in offsets]
    states, scores = np.zeros(len(q), dtype=np.uint8), []
    for a, b in zip(off[:-1], off[1:]):
        st, sc = viterbi(q[a:b], qlog_trans, qlog_init)
        states[a:b] = st
        scores.append(sc)
    return states, scores


# ---- (ii) ----------------------------------------------------------------------------------------------------------------
def forward_backward(E, trans, init):
    """One record: (gamma (n, S), xi (S, S), gamma_0 (S,), log evidence) in longdouble; zeros for n = 0."""
    E = np.asarray(E, dtype=np.float64)
    n, S = E.shape
    A, pi = np.asarray(trans, dtype=np.float64).astype(LD), np.asarray(init, dtype=np.float64).astype(LD)
    if n == 0:
        return np.zeros((0, S), dtype=LD), np.zeros((S, S), dtype=LD), np.zeros(S, dtype=LD), LD(0)
    e = np.exp(relative(E).astype(LD))
    al, c = np.zeros((n, S), dtype=LD), np.zeros(n, dtype=LD)
    v = pi * e[0]
    c[0] = v.sum()
    al[0] = v / c[0]
    for t in range(1, n):
        v = (al[t - 1] @ A) * e[t]
        c[t] = v.sum()
        al[t] = v / c[t]
    be = np.ones((n, S), dtype=LD)
    xi = np.zeros((S, S), dtype=LD)
    for t in range(n - 2, -1, -1):
        w = e[t + 1] * be[t + 1]
        xi += al[t][:, None] * A * w[None, :] / c[t + 1]
        be[t] = (A @ w) / c[t + 1]
    gamma = al * be
    gamma /= gamma.sum(axis=1, keepdims=True)
    return gamma, xi, gamma[0].copy(), np.log(c).sum() + E.max(axis=1).astype(LD).sum()


def expect(E, offsets, trans, init, counts=None):
    """Over the records: dict of gamma (n, S), xi, gamma0, log_evidence (total), log_evidence_rec (R,), and with ``counts``
    T (S, D) and Ns (S,) -- longdouble."""
    E = np.asarray(E, dtype=np.float64)
    S = E.shape[1]
    off = [int(o) for o in offsets]
    gamma = np.zeros(E.shape, dtype=LD)
    xi, g0, rec = np.zeros((S, S), dtype=LD), np.zeros(S, dtype=LD), []
    for a, b in zip(off[:-1], off[1:]):
        g, x, z, le = forward_backward(E[a:b], trans, init)
        gamma[a:b] = g
        xi += x
        g0 += z
        rec.append(le)
    out = dict(gamma=gamma, xi=xi, gamma0=g0, log_evidence_rec=np.array(rec, dtype=LD), log_evidence=np.sum(np.array(rec, dtype=LD)))
    if counts is not None:
        out["T"] = gamma.T @ np.asarray(counts).astype(LD)
        out["Ns"] = gamma.sum(axis=0)
    return out


# ---- (iii) ---------------------------------------------------------------------------------------------------------------
def brute_force(E, trans, init, qlog_trans, qlog_init):
    """One record, n <= 7 and S <= 3, over all S^n paths: (gamma (n, S), xi (S, S), log evidence, best integer score, the
    list of paths that reach it)."""
    E = np.asarray(E, dtype=np.float64)
    n, S = E.shape
    assert 1 <= n <= 7 and S <= 3
    A, pi = np.asarray(trans, dtype=np.float64).astype(LD), np.asarray(init, dtype=np.float64).astype(LD)
    e, q = np.exp(relative(E).astype(LD)), quantise(E)
    gamma, xi, total = np.zeros((n, S), dtype=LD), np.zeros((S, S), dtype=LD), LD(0)
    best, paths = None, []
    for path in itertools.product(range(S), repeat=n):
        p, sc = pi[path[0]] * e[0][path[0]], int(qlog_init[path[0]]) + q[0][path[0]]
        for t in range(1, n):
            p = p * A[path[t - 1]][path[t]] * e[t][path[t]]
            sc += int(qlog_trans[path[t - 1]][path[t]]) + q[t][path[t]]
        total += p
        for t in range(n):
            gamma[t][path[t]] += p
            if t:
                xi[path[t - 1]][path[t]] += p
        if best is None or sc > best:
            best, paths = sc, [path]
        elif sc == best:
            paths.append(path)
    return gamma / total, xi / total, np.log(total) + E.max(axis=1).astype(LD).sum(), best, paths


# ---- the start rule and the M-step ---------------------------------------------------------------------------------------------
def blocks(counts, offsets, block):
    """The pooled counts (n_blocks, D) int64 of every record's blocks of ``block`` consecutive windows (a record's last
    block may be shorter; blocks never cross records)."""
    c = np.asarray(counts).astype(np.int64)
    off = [int(o) for o in offsets]
    rows = []
    for a, b in zip(off[:-1], off[1:]):
        for s in range(a, b, int(block)):
            rows.append(c[s:min(s + int(block), b)].sum(axis=0))
    return np.array(rows, dtype=np.int64).reshape(len(rows), c.shape[1])


def start(counts, offsets, n_states, block=20, pseudocount=0.5):
    """(log profiles (S, D), block indices): the first block with k-mers, then S - 1 times the block whose best per-k-mer
    log-likelihood under the smoothed profiles of the chosen blocks is lowest (ties: the lowest index)."""
    P = blocks(counts, offsets, block)
    tot = P.sum(axis=1)
    live = [i for i in range(len(P)) if tot[i] > 0]
    if len(live) < n_states:
        raise ValueError("fewer blocks with k-mers than states")
    smooth = lambda idx: np.log((P[idx] + pseudocount) / (P[idx].sum(axis=1, keepdims=True) + P.shape[1] * pseudocount))
    chosen = [live[0]]
    while len(chosen) < n_states:
        lp = smooth(chosen)
        worst, at = None, None
        for i in live:
            if i in chosen:
                continue
            best = max(float(np.dot(P[i].astype(np.float64), lp[s])) for s in range(len(chosen))) / float(tot[i])
            if worst is None or best < worst:
                worst, at = best, i
        chosen.append(at)
    return smooth(chosen), chosen


def m_step(T, xi, gamma0, pseudocount, prior_counts=0.0, p_start='fixed', trans=None, init=None):
    """(log profiles, trans, init) of the M-step, operation by operation."""
    T, xi = np.asarray(T, dtype=np.float64), np.asarray(xi, dtype=np.float64)
    S, D = T.shape
    logp = np.log((T + pseudocount) / (T.sum(axis=1, keepdims=True) + D * pseudocount))

    def normalised(v, keep):
        s = v.sum()
        if not s > 0:
            return np.array(keep, dtype=np.float64)
        p = np.maximum(v / s, 1e-12)
        return p / p.sum()

    x = xi + np.broadcast_to(np.asarray(prior_counts, dtype=np.float64), (S, S))
    A = np.array([normalised(x[i], None if trans is None else np.asarray(trans)[i]) for i in range(S)])
    pi = init if p_start == 'fixed' else normalised(np.asarray(gamma0, dtype=np.float64), init)
    return logp, A, pi


# ---- bounds ------------------------------------------------------------------------------------------------------------------
def chain_error(n, S):
    return (n * (2.0 * S + 1.0 + 2.0 * EXP_ULP) + 4.0 * S + 8.0) * U


def posterior_bound(n, S):
    """B(n, S) for a record of n windows."""
    return 2.0 * chain_error(n, S)


def evidence_bound(M, S, log_evidence):
    """For one record with row maxima ``M`` (n,)."""
    n, m = len(M), float(np.abs(np.asarray(M, dtype=np.float64)).sum())
    return chain_error(n, S) + n * U * m + 8.0 * U * (abs(float(log_evidence)) + m + 1.0)


def check_posterior(got, exact, n_longest, S, what=""):
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=LD)
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(LD) - exact)
    bound = LD(posterior_bound(n_longest, S)) * exact + LD(FLOOR)
    bad = err > bound
    assert not bad.any(), "%s: %d posteriors outside B(n, S); worst error / bound %.3g" % (
        what, int(bad.sum()), float((err / bound).max()))
    return float((err / bound).max())


def check_sums(got, exact, n_longest, S, terms, floor_terms, what=""):
    """A sum of ``terms`` positive terms each inside B: (B + (terms + 2) u) exact + floor_terms FLOOR."""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=LD)
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(LD) - exact)
    bound = LD(posterior_bound(n_longest, S) + (terms + 2.0) * U) * exact + LD(FLOOR) * LD(floor_terms)
    assert not (err > bound).any(), "%s: worst error / bound %.3g" % (what, float((err / np.maximum(bound, LD(1e-4000))).max()))


# ---- the sequences of the fit tests ----------------------------------------------------------------------------------------------
SMALL_BOUNDS = [0, 12000, 20000, 30000, 40000]


def window_counts(seq, window=500, k=4):
    """4-mer counts (len(seq) // window, 256) int64 of the consecutive windows of ``seq`` (the project's column order)."""
    d = np.array(["ATGC".index(ch) for ch in seq])
    km = sum(d[i:len(d) - (k - 1) + i] * 4 ** (k - 1 - i) for i in range(k))
    n = len(seq) // window
    return np.array([np.bincount(km[i * window:i * window + window - (k - 1)], minlength=4 ** k) for i in range(n)],
                    dtype=np.int64)


def small_rows():
    from tests import helpers
    g = helpers.load_npz("ref_features.npz")
    pos, neg = g["pos_counts"].astype(np.int64), g["neg_counts"].astype(np.int64)
    return [neg[2000], pos[2200], neg[100], neg[2000]]


def small_sequence(seed):
    """The "small" sequence: 40 kb in four pieces from three order-3 chains (negative rows 2000 and 100, positive row 2200 of
    the golden reference), the first and the last piece from the same chain."""
    from tests import segment_ref
    return segment_ref.chain_sequence(np.random.default_rng(seed), small_rows(), SMALL_BOUNDS, SMALL_BOUNDS[-1])


def changes(state, step=500):
    """The base positions at which the path changes state."""
    return [int(i) * step for i in np.flatnonzero(np.diff(np.asarray(state).astype(np.int64))) + 1]


# ---- the statement in the place of the device (tests/test_compose_host.py) ----------------------------------------------------------
class StatementEStep(object):
    """What compose._estep returns, computed by this module in longdouble and rounded to float64."""

    def __init__(self, counts_or_batch, offsets, n_states, batch_rows=0):
        self.host = np.ascontiguousarray(counts_or_batch, dtype=np.uint32)
        self.offsets = np.asarray(offsets, dtype=np.uint64)
        self.n, self.D, self.S = self.host.shape[0], self.host.shape[1], int(n_states)

    def counts(self):
        return self.host

    def _emissions(self, log_profiles, temper):
        return exact_emissions(self.host, log_profiles, temper).astype(np.float64)

    def __call__(self, log_profiles, trans, init, temper):
        E = self._emissions(log_profiles, temper)
        o = expect(E, self.offsets, trans, init, self.host)
        f = lambda v: np.asarray(v, dtype=np.float64)
        return f(o["T"]), f(o["Ns"]), f(o["xi"]), f(o["gamma0"]), float(o["log_evidence"])

    def decode(self, log_profiles, trans, init, temper):
        E = self._emissions(log_profiles, temper)
        o = expect(E, self.offsets, trans, init)
        states, scores = viterbi_records(E, self.offsets, quantise_log(trans), quantise_log(init))
        return (states, np.asarray(o["gamma"], dtype=np.float64), np.asarray(o["log_evidence_rec"], dtype=np.float64),
                np.array(scores, dtype=np.int64))

    def close(self):
        pass
