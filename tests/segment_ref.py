"""The two-state hidden Markov decode (phamers_amd/segment.py, csrc/segment.hip) restated in
NumPy and plain Python, and the tolerance the device's float64 forward-backward is held to.

    states 0 = host, 1 = phage;  emission e_t = (1, exp(x_t));  A = [[1 - a, a], [b, 1 - b]];  start pi

(i)   ``viterbi``            the plain left-to-right max-plus recurrence on Python ints (units of 2^-16 nat), ties to the
                             predecessor with the smaller state, a tie at the final step to the smaller state
(ii)  ``forward_backward``   posterior, 1 - posterior and log_odds in np.longdouble, sequential, log domain.  The two
                             vectors are renormalised at every step (the shifts summed apart), so every logarithm it adds
                             stays of magnitude |x_t| + |log a| and the statement's own error is about n 2^-63 relative
                             on the posterior: 2^-10 of the bound below.
(iii) ``brute_force``        all 2^n paths (n <= 12): the best path by exact integer score under the recurrence's tie rule,
                             and the marginals and the evidence as longdouble sums
(iv)  ``posterior_bound`` / ``log_odds_bound``   see below

The tie rule, restated for (iii): the recurrence picks the final state first (the smaller of two that tie), then at every
step backwards the smaller predecessor among those that attain the maximum -- every such predecessor continues an optimal
path, so the path chosen is, of all paths with the maximal score, the smallest one read from its END.

Error bound of the float64 forward-backward (derived; u = 2^-53).  The device works in the probability domain: every
quantity is a sum of products of positive numbers, so relative errors only add.  One step of a forward or backward
recurrence, or of a tile's matrix product, computes (f A + f' A') e: two products, one sum, one product with the emission
-- 4 roundings, (1 + u) each, fused or not -- and the emission exp(-|x_t|) itself, whose argument is exact and whose value
errs by EXP_ULP ulp <= 2 EXP_ULP u relative.  Rescaling by a power of two is exact.  Carrying a tile's product into the
running vector costs 3 roundings per tile of 64 steps, less than 1/16 per step.  alpha_t sees t steps and beta_t the other
n - t, so each of p_s = alpha_t(s) beta_t(s) carries at most n (4 + 2 EXP_ULP + 1/16) u + 2 u, and the quotient
p_1 / (p_0 + p_1) at most twice the larger of the two, plus a sum and a division.  With the second-order terms (n u < 2^-22
for 2^31 windows: 1 %):

    |posterior - exact| <= B(n) * exact + FLOOR,      B(n) = 2 (n (5 + 2 EXP_ULP) + 16) u
    |(1 - posterior) - (1 - exact)| <= B(n)           (the same relative error, of a number <= 1)

FLOOR = 2^-1000 is the format's, not the method's: exp(-|x|) below 2^-1022 is subnormal or 0 ("certain"), and a component
2^-1022 below its partner is rounded absolutely when the pair is rescaled; transition probabilities down to 2^-60 move
such a value by less than 2^-1000.

log_odds = (E ln 2 + log m) + S with E the integer exponent, m in [1/2, 1) and S = sum_t max(x_t, 0) (the emissions enter
scaled by exp(-max(x_t, 0))).  The evidence m 2^E carries n (4 + 2 EXP_ULP + 1/16) u relative, which is absolute on its
logarithm; S is a sum of n non-negative terms in order: n u S; the product E ln 2, log m (a few ulp of a value <= ln 2) and
the two sums add a few u of |E ln 2| <= |log_odds| + S + 1:

    |log_odds - exact| <= (n (5 + 2 EXP_ULP) + 16) u + n u S + 8 u (|log_odds| + S + 1)

EXP_ULP: the one constant that cannot be derived.  The device library's documentation is not part of the ROCm installation
this was written against, so it was measured once on the MI355X (profiles/segment/README.md): the device's exp(-|x|) against
longdouble exp over the x values of tests/test_gpu_segment.py and a sweep of [-745, 745] (675 625 values; 664 812 of the
results normal numbers).  Measured worst: 0.841 ulp, recorded as EXP_ULP_MEASURED = 0.85; the bound takes twice that.
"""
import itertools

import numpy as np

U = 2.0 ** -53
QUANT_BITS = 16
CLAMP = 2.0 ** 15
EXP_ULP_MEASURED = 0.85
EXP_ULP = 2.0 * EXP_ULP_MEASURED
FLOOR = 2.0 ** -1000
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the extended statement needs a longdouble wider than float64"


def quantise(v):
    """rint(clip(v, -2^15, 2^15) 2^16) as Python ints (a list), ties to even."""
    return [int(q) for q in np.rint(np.clip(np.atleast_1d(np.asarray(v, dtype=np.float64)), -CLAMP, CLAMP) * 2.0 ** QUANT_BITS)]


def parameters(a, b, s=None):
    """(trans (4,), init (2,)) float64 as segment.parameters builds them."""
    s = a / (a + b) if s is None else s
    return np.array([1.0 - a, a, b, 1.0 - b]), np.array([1.0 - s, s])


def biased_evidence(rng, n, scale=3.0, run=37, bias=2.0):
    """Random x of scale ``scale`` with runs of ``run`` windows biased to + or -, so that paths switch."""
    sign = np.repeat(rng.choice([-bias, bias], size=n // run + 1), run)[:n]
    return scale * rng.standard_normal(n) + sign


def chain_sequence(rng, rows, bounds, length):
    """A sequence of ``length`` bases drawn from order-3 Markov chains: piece i, the bases [bounds[i], bounds[i + 1]), from
    the chain of the 4-mer count row rows[i] -- ``(row + 0.5)`` per 3-mer context, in the project's column order (first base
    most significant, digits of 'ATGC').  One ``rng.random(length)`` draw; the first three bases are uniform."""
    u = rng.random(length)
    cums = []
    for row in rows:
        w = np.asarray(row, dtype=np.float64).reshape(64, 4) + 0.5
        cums.append(np.cumsum(w / w.sum(axis=1, keepdims=True), axis=1).tolist())
    out = [int(4 * u[i]) for i in range(3)]
    piece = 0
    for i in range(3, length):
        while i >= bounds[piece + 1]:
            piece += 1
        c = cums[piece][out[i - 3] * 16 + out[i - 2] * 4 + out[i - 1]]
        out.append(0 if u[i] < c[0] else 1 if u[i] < c[1] else 2 if u[i] < c[2] else 3)
    return "".join("ATGC"[d] for d in out)


def runs(flags):
    """[(first, last + 1)] of the runs of true entries."""
    d = np.diff(np.concatenate(([0], np.asarray(flags, dtype=np.int8), [0])))
    return [(int(a), int(b)) for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1))]


# ---- (i) -----------------------------------------------------------------------------------------------------------------
def viterbi(qx, qlog_trans, qlog_init):
    """(states (n,) uint8, score int) of the integer evidence ``qx`` (Python ints)."""
    qa = [int(v) for v in qlog_trans]
    n = len(qx)
    if n == 0:
        return np.zeros(0, dtype=np.uint8), 0
    d = [int(qlog_init[0]), int(qlog_init[1]) + int(qx[0])]
    back = []
    for t in range(1, n):
        c0 = (d[0] + qa[0], d[1] + qa[2])          # into state 0 from 0, 1
        c1 = (d[0] + qa[1], d[1] + qa[3])          # into state 1
        k0, k1 = int(c0[1] > c0[0]), int(c1[1] > c1[0])
        back.append((k0, k1))
        d = [c0[k0], c1[k1] + int(qx[t])]
    s = int(d[1] > d[0])
    score = d[s]
    states = np.empty(n, dtype=np.uint8)
    states[n - 1] = s
    for t in range(n - 1, 0, -1):
        s = back[t - 1][s]
        states[t - 1] = s
    return states, score


# ---- (ii) ----------------------------------------------------------------------------------------------------------------
def forward_backward(x, trans, init):
    """(posterior (n,), one_minus_posterior (n,), log_odds) in longdouble."""
    x = np.asarray(x, dtype=LD)
    n = x.shape[0]
    if n == 0:
        return np.zeros(0, dtype=LD), np.zeros(0, dtype=LD), LD(0)
    lA = np.log(np.asarray(trans, dtype=LD).reshape(2, 2))
    lpi = np.log(np.asarray(init, dtype=LD))
    em = np.zeros((n, 2), dtype=LD)
    em[:, 1] = x
    la, lb = np.empty((n, 2), dtype=LD), np.empty((n, 2), dtype=LD)
    shift = LD(0)
    for t in range(n):
        v = (lpi if t == 0 else np.logaddexp(la[t - 1, 0] + lA[0], la[t - 1, 1] + lA[1])) + em[t]
        m = v.max()
        la[t] = v - m
        shift += m
    log_odds = shift + np.logaddexp(la[n - 1, 0], la[n - 1, 1])
    lb[n - 1] = 0
    for t in range(n - 1, 0, -1):
        w = em[t] + lb[t]
        v = np.logaddexp(lA[:, 0] + w[0], lA[:, 1] + w[1])
        lb[t - 1] = v - v.max()
    g = la + lb
    total = np.logaddexp(g[:, 0], g[:, 1])
    return np.exp(g[:, 1] - total), np.exp(g[:, 0] - total), log_odds


# ---- (iii) ---------------------------------------------------------------------------------------------------------------
def brute_force(x, trans, init, qlog_trans, qlog_init):
    """Over all 2^n paths (n <= 12): (best path (n,) uint8, its integer score, posterior (n,) longdouble, log_odds)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    assert 1 <= n <= 12
    qx, qa, qp = quantise(x), [int(v) for v in qlog_trans], [int(v) for v in qlog_init]
    A, pi, w1 = np.asarray(trans, dtype=LD).reshape(2, 2), np.asarray(init, dtype=LD), np.exp(x.astype(LD))
    best, total, marginal = None, LD(0), np.zeros(n, dtype=LD)
    for path in itertools.product((0, 1), repeat=n):
        score, p = qp[path[0]] + path[0] * qx[0], pi[path[0]] * (w1[0] if path[0] else LD(1))
        for t in range(1, n):
            score += qa[2 * path[t - 1] + path[t]] + path[t] * qx[t]
            p = p * A[path[t - 1], path[t]] * (w1[t] if path[t] else LD(1))
        key = (-score, path[::-1])
        if best is None or key < best[0]:
            best = (key, path, score)
        total += p
        marginal += p * np.array(path, dtype=LD)
    return np.array(best[1], dtype=np.uint8), best[2], marginal / total, np.log(total)


# ---- (iv) ----------------------------------------------------------------------------------------------------------------
def posterior_bound(n):
    return 2.0 * (n * (5.0 + 2.0 * EXP_ULP) + 16.0) * U


def log_odds_bound(x, log_odds):
    x = np.asarray(x, dtype=np.float64)
    n, S = x.shape[0], float(np.maximum(x, 0.0).sum())
    return (n * (5.0 + 2.0 * EXP_ULP) + 16.0) * U + n * U * S + 8.0 * U * (abs(float(log_odds)) + S + 1.0)


def check(posterior, log_odds, x, trans, init, what=""):
    """Asserts the three checks of (iv) against statement (ii); returns the statement."""
    want, want_1m, want_lo = forward_backward(x, trans, init)
    n = len(want)
    got = np.asarray(posterior).astype(LD)
    if n:
        B = posterior_bound(n)
        err = np.abs(got - want)
        worst = int(np.argmax(err / (B * want + FLOOR)))
        assert (err <= B * want + FLOOR).all(), "%s posterior: window %d is %r, statement %r, relative bound %.3e" % (
            what, worst, posterior[worst], want[worst], B)
        err1 = np.abs((LD(1) - got) - want_1m)
        worst = int(np.argmax(err1))
        assert (err1 <= B).all(), "%s 1 - posterior: window %d off by %.3e, bound %.3e" % (what, worst, float(err1[worst]), B)
    bl = log_odds_bound(x, want_lo)
    assert abs(LD(log_odds) - want_lo) <= bl, "%s log_odds %r, statement %r, bound %.3e" % (what, log_odds, want_lo, bl)
    return want, want_1m, want_lo
