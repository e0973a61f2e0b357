"""The fit of the segmentation chain (phamers_amd/segment.py ``expected_counts`` / ``fit``, csrc/segment.hip, DESIGN.md section
4.23) restated in NumPy, and the tolerance the device's float64 E-step is held to.  The model is tests/segment_ref.py's:

    states 0 = host, 1 = phage;  emission e_t = (1, exp(x_t));  A = [[1 - a, a], [b, 1 - b]];  start pi

    xi(i->j)   = sum_{t >= 1} P(s_{t-1} = i, s_t = j | x)        four numbers per record
    gamma_0(s) = P(s_0 = s | x)                                  two numbers per record

(i)   ``expected``       the E-step in np.longdouble, sequential, probability domain: alpha and beta are renormalised to
                         sum 1 at every step and every step's four terms alpha_{t-1}(i) A_ij e_t(j) beta_t(j) by their own
                         sum, so nothing under- or overflows and the statement's own error is about n 2^-63 relative.  It
                         takes (R, n) tracks of equal length side by side.
(ii)  ``brute_force``    all 2^n paths (n <= 12): xi, gamma_0 and the log evidence as longdouble sums
(iii) ``m_step``         the M-step in float64, operation for operation what include/phamers_hip.h specifies
(iv)  ``tree_sum``       the reduction over the records: blocks of 256 consecutive rows, a row past the end +0.0, within a
                         block v[i] += v[i + s] for s = 128, 64, .. 1, the block results by the same rule until one is left
(v)   the bounds, derived below

Error bound of the float64 E-step (derived; u = 2^-53; the constants of tests/segment_ref.py).  There alpha_t and beta_t are
shown to carry at most (4 + 2 EXP_ULP + 1/16) u relative per step they have seen; alpha_{t-1} has seen t - 1 steps and
beta_t the n - 1 - t after it, together fewer than n.  A term w_ij = (alpha_{t-1}(i) A_ij) (e_t(j) beta_t(j)) adds three
roundings and the emission's 2 EXP_ULP u:

    w_ij carries at most  d = (n (4 + 2 EXP_ULP + 1/16) + 3 + 2 EXP_ULP) u.

The step's sum s = (w00 + w01) + (w10 + w11) is a sum of positive numbers: the relative error of its terms (<= d) and two
additions on every term's way.  The share w_ij (1 / s) adds the reciprocal's rounding and the product's: at most
2 d + 4 u.  The shares of the record's n - 1 steps are added in step order inside a tile and the tile sums in tile order: a
share passes fewer than n additions of positive numbers, n u.  Rounded up as segment_ref.posterior_bound rounds (which is
2 (n (5 + 2 EXP_ULP) + 16) u >= 2 d + 4 u):

    |xi(i->j) - exact| <= XI(n) * exact + n FLOOR,        XI(n) = posterior_bound(n) + (n + 16) u
    |gamma_0(s) - exact| <= posterior_bound(n) * exact + FLOOR          (one share, no sum)

FLOOR as there: a component 2^-1022 below its partner is rounded absolutely; every step may add one such error.

The totals add the records' values through the tree (iv): a value passes 8 additions per level, ``tree_levels(R)`` levels.
All six columns are positive, so with n_max the longest record

    |total - exact| <= (XI(n_max) + 8 levels u) * exact + N FLOOR       (N = all windows)

and the log evidence, whose terms have either sign,

    |L - exact| <= sum_r log_odds_bound(r) + 8 levels u sum_r |log_odds_r|.

No constant here was tuned against the device; EXP_ULP is segment_ref's (measured there once, doubled).
"""
import itertools

import numpy as np

from tests import segment_ref as ref

U, FLOOR, LD = ref.U, ref.FLOOR, ref.LD
BLOCK = 256
P_MIN, P_MAX = 1e-12, 1.0 - 1e-12
FIXED, FREE, STATIONARY = 0, 1, 2
CONVERGED, CLAMPED, NO_TRANSITIONS = 1, 2, 4


# ---- (i) -----------------------------------------------------------------------------------------------------------------
def expected(x, trans, init):
    """(xi (R, 4), gamma0 (R, 2), log_odds (R,)) in longdouble of the tracks ``x`` (R, n) -- or (n,), read as one record.
    Columns of xi: 0->0, 0->1, 1->0, 1->1."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64)).astype(LD)
    R, n = x.shape
    xi, g0, lo = np.zeros((R, 4), dtype=LD), np.zeros((R, 2), dtype=LD), np.zeros(R, dtype=LD)
    if n == 0:
        return xi, g0, lo
    A, pi = np.asarray(trans, dtype=LD).reshape(2, 2), np.asarray(init, dtype=LD)
    m = np.exp(-np.abs(x))                                           # the emission scaled by exp(-max(x, 0))
    e = np.stack((np.where(x > 0, m, LD(1)), np.where(x > 0, LD(1), m)), axis=2)     # (R, n, 2)
    lo += np.maximum(x, 0).sum(axis=1)
    alpha, beta = np.empty((n, R, 2), dtype=LD), np.empty((n, R, 2), dtype=LD)
    for t in range(n):
        v = (pi[None, :] if t == 0 else alpha[t - 1] @ A) * e[:, t]
        s = v.sum(axis=1)
        alpha[t] = v / s[:, None]
        lo += np.log(s)
    beta[n - 1] = LD(0.5)
    for t in range(n - 1, 0, -1):
        v = (e[:, t] * beta[t]) @ A.T
        beta[t - 1] = v / v.sum(axis=1)[:, None]
    g = alpha[0] * beta[0]
    g0[:] = g / g.sum(axis=1)[:, None]
    for t in range(1, n):
        w = alpha[t - 1][:, :, None] * A[None, :, :] * (e[:, t] * beta[t])[:, None, :]      # (R, 2, 2)
        xi += (w / w.sum(axis=(1, 2))[:, None, None]).reshape(R, 4)
    return xi, g0, lo


# ---- (ii) ----------------------------------------------------------------------------------------------------------------
def brute_force(x, trans, init):
    """Over all 2^n paths (1 <= n <= 12): (xi (4,), gamma0 (2,), log evidence) as longdouble sums."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    assert 1 <= n <= 12
    A, pi, w1 = np.asarray(trans, dtype=LD).reshape(2, 2), np.asarray(init, dtype=LD), np.exp(x.astype(LD))
    total, xi, g0 = LD(0), np.zeros(4, dtype=LD), np.zeros(2, dtype=LD)
    for path in itertools.product((0, 1), repeat=n):
        p = pi[path[0]] * (w1[0] if path[0] else LD(1))
        for t in range(1, n):
            p = p * A[path[t - 1], path[t]] * (w1[t] if path[t] else LD(1))
        total += p
        g0[path[0]] += p
        for t in range(1, n):
            xi[2 * path[t - 1] + path[t]] += p
    return xi / total, g0 / total, np.log(total)


# ---- (iii) ---------------------------------------------------------------------------------------------------------------
def _clamp(p, status):
    if p < P_MIN:
        return P_MIN, status | CLAMPED
    if p > P_MAX:
        return P_MAX, status | CLAMPED
    return p, status


def m_step(totals, params, prior_counts=(0.0, 0.0, 0.0, 0.0), start_mode=STATIONARY):
    """((a, b, p_start), status bits) after one M-step on ``totals`` = (N00, N01, N10, N11, G0, G1) from ``params`` =
    (a, b, p_start): float64, one IEEE operation per sign written."""
    N = [np.float64(v) for v in totals]
    c = [np.float64(v) for v in prior_counts]
    a, b, s = (np.float64(v) for v in params)
    status = 0
    n00, n01, n10, n11 = N[0] + c[0], N[1] + c[1], N[2] + c[2], N[3] + c[3]
    if n00 + n01 > 0:
        a, status = _clamp(n01 / (n00 + n01), status)
    else:
        status |= NO_TRANSITIONS
    if n10 + n11 > 0:
        b, status = _clamp(n10 / (n10 + n11), status)
    else:
        status |= NO_TRANSITIONS
    if start_mode == FREE:
        if N[4] + N[5] > 0:
            s, status = _clamp(N[5] / (N[4] + N[5]), status)
    elif start_mode == STATIONARY:
        s, status = _clamp(a / (a + b), status)
    return (float(a), float(b), float(s)), status


def expected_records(tracks, trans, init):
    """``expected`` of equal-length tracks (R, n), or of a list of 1-D tracks of any lengths, one by one."""
    if isinstance(tracks, np.ndarray) and tracks.ndim == 2:
        return expected(tracks, trans, init)
    parts = [expected(t, trans, init) for t in tracks]
    if not parts:
        return np.zeros((0, 4), dtype=LD), np.zeros((0, 2), dtype=LD), np.zeros(0, dtype=LD)
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def em(x, a, b, s, start_mode=STATIONARY, prior_counts=(0.0, 0.0, 0.0, 0.0), max_iter=200, tol=1e-8):
    """The loop of phk_segment_fit on statement (i), tracks ``x`` as ``expected_records`` takes them: (trace rows [(a, b, s,
    totals (6,), L)], n_iter, status).  The totals are longdouble sums rounded to float64 for the M-step."""
    params, status, trace = (float(a), float(b), float(s)), 0, []
    while True:
        xi, g0, lo = expected_records(x, ref.parameters(params[0], params[1], params[2])[0], [1.0 - params[2], params[2]])
        totals = np.concatenate((xi.sum(axis=0), g0.sum(axis=0))).astype(np.float64)
        trace.append(params + (totals, float(lo.sum())))
        i = len(trace) - 1
        if i > 0 and trace[i][4] - trace[i - 1][4] <= tol * max(1.0, abs(trace[i][4])):
            status |= CONVERGED
            break
        if i == max_iter:
            break
        params, bits = m_step(totals, params, prior_counts, start_mode)
        status |= bits
    if len(trace) > 1 and trace[-1][4] < trace[-2][4]:
        trace.pop()
    return trace, len(trace) - 1, status


# ---- (iv) ----------------------------------------------------------------------------------------------------------------
def tree_levels(R):
    levels, m = 1, -(-R // BLOCK)
    while m > 1:
        levels, m = levels + 1, -(-m // BLOCK)
    return levels


def tree_sum(values):
    """The column sums of ``values`` (R, C) float64 by the device's tree, in float64.  (R, C) with R = 0 gives zeros."""
    v = np.array(values, dtype=np.float64, ndmin=2)
    if v.shape[0] == 0:
        return np.zeros(v.shape[1])
    while True:
        blocks = -(-v.shape[0] // BLOCK)
        padded = np.zeros((blocks * BLOCK, v.shape[1]))
        padded[:v.shape[0]] = v
        w = padded.reshape(blocks, BLOCK, v.shape[1])
        s = BLOCK // 2
        while s:
            w[:, :s] += w[:, s:2 * s]
            s //= 2
        v = w[:, 0].copy()
        if blocks == 1:
            return v[0]


# ---- (v) -----------------------------------------------------------------------------------------------------------------
def xi_bound(n):
    return ref.posterior_bound(n) + (n + 16.0) * U


def check_record(counts, log_odds, x, trans, init, what="", want=None):
    """Asserts a record's six counts (xi00, xi01, xi10, xi11, g0, g1) and log_odds against statement (i) within (v);
    returns the statement's (xi, gamma0, log_odds)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    xi, g0, lo = want if want is not None else tuple(v[0] for v in expected(x, trans, init))
    got = np.asarray(counts, dtype=np.float64).astype(LD)
    assert np.isfinite(np.asarray(counts)).all() and (np.asarray(counts) >= 0).all(), (what, counts)
    err = np.abs(got[:4] - xi)
    assert (err <= xi_bound(n) * xi + n * FLOOR).all(), "%s xi: got %r, statement %r, relative bound %.3e" % (
        what, counts[:4], xi, xi_bound(n))
    err = np.abs(got[4:] - g0)
    assert (err <= ref.posterior_bound(n) * g0 + FLOOR).all(), "%s gamma_0: got %r, statement %r, relative bound %.3e" % (
        what, counts[4:], g0, ref.posterior_bound(n))
    bl = ref.log_odds_bound(x, lo)
    assert abs(LD(log_odds) - lo) <= bl, "%s log_odds %r, statement %r, bound %.3e" % (what, log_odds, lo, bl)
    return xi, g0, lo


def check_totals(totals, log_evidence, x, trans, init, what=""):
    """Asserts the six totals and the log evidence of equal-length tracks ``x`` (R, n) against statement (i) within (v);
    returns the statement's totals, its log evidence and the bound on the latter."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    R, n = x.shape
    xi, g0, lo = expected(x, trans, init)
    want = np.concatenate((xi.sum(axis=0), g0.sum(axis=0)))
    levels = tree_levels(R)
    bound = (xi_bound(n) + 8.0 * levels * U) * want + R * n * FLOOR
    err = np.abs(np.asarray(totals, dtype=np.float64).astype(LD) - want)
    assert (err <= bound).all(), "%s totals: got %r, statement %r, relative bound %.3e" % (
        what, totals, want.astype(np.float64), xi_bound(n) + 8.0 * levels * U)
    bl = evidence_bound(x, lo)
    assert abs(LD(log_evidence) - lo.sum()) <= bl, "%s log evidence %r, statement %r, bound %.3e" % (
        what, log_evidence, lo.sum(), bl)
    return want, lo.sum(), bl


def evidence_bound(x, log_odds):
    """The bound on the sum of the records' log_odds: tracks ``x`` (R, n), the statement's ``log_odds`` (R,)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    return sum(ref.log_odds_bound(x[r], log_odds[r]) for r in range(x.shape[0])) + \
        8.0 * tree_levels(x.shape[0]) * U * float(np.abs(log_odds).sum())


def sample_chain(rng, records, n, a, b):
    """``records`` tracks of ``n`` windows from the chain (a, b) started stationary; the score of a window is
    x = 2 N(+-1, 1): the exact log-likelihood ratio of N(1, 1) against N(-1, 1).  -> x (records, n), states (records, n)."""
    states = np.empty((records, n), dtype=np.int8)
    u = rng.random((records, n))
    states[:, 0] = u[:, 0] < a / (a + b)
    for t in range(1, n):
        states[:, t] = np.where(states[:, t - 1] == 1, u[:, t] >= b, u[:, t] < a)
    return 2.0 * (rng.standard_normal((records, n)) + (2.0 * states - 1.0)), states
