"""The statement of the boundary confidence: the exact part in Python ints, the five sums in
``numpy.longdouble``, and the bounds a float64 evaluation is held to.

With d, P, position = p* and P* = P(p*) as in tests/refine_ref.py, the candidates p = lo .. hi (P(lo) = 0, n = hi - lo + 1) and
drop_q >= 0 an integer in units of 2^-16 nat:

    lower / upper = the smallest / largest p with P(p) >= P* - drop_q;  n_within = the number of such p
    w(p)     = exp(-(P* - P(p)) 2^-16), and 0 where P* - P(p) > 700 * 2^16 (compared as integers)
    Z        = sum_p w(p)                       M = sum of w(p) over lower <= p <= upper
    S1_left  = sum_{p < p*} (p* - p) w(p)       S1_right = sum_{p > p*} (p - p*) w(p)       S2 = sum_p (p - p*)^2 w(p)
    log_z = log Z, mass_at_position = 1 / Z, mass_within = M / Z, mean_offset = (S1_right - S1_left) / Z,
    rms_distance = sqrt(S2 / Z)

Here the sums are added in increasing p in longdouble (64-bit mantissa; asserted by tests/segment_ref.py).

The bound (u = 2^-53; derived, no constant tuned against the device).  Below the cut P* - P(p) is an integer below 2^53 and
the argument of exp that integer times 2^-16: exact in float64.  So a float64 weight carries the error of exp alone,
EXP_ULP ulp <= 2 EXP_ULP u relative (EXP_ULP: tests/segment_ref.py, the one measured constant, doubled there), and every
weight is a normal number (>= e^-700): nothing underflows, no absolute floor is needed.  The factor p - p* is an integer
below 2^53, exact; its product with w rounds once (1 u).  (p - p*)^2 is formed in int64 (< 2^61) and converted once (1 u),
its product rounds once more: 2 u.  A sum of n non-negative terms, in any order and any bracketing, passes each term through
at most n - 1 additions: (n - 1) u to first order.  Together, to first order, at most (n + 2 EXP_ULP + 1) u relative.  What
is left: second order, (r^2 with r <= 2^-22 for n <= 2^30 + 1: below r 2^-10); this statement's own error -- n additions,
two roundings and an exp in longdouble, (n + 4) 2^-64 = (n + 4) u 2^-11 relative.  Hence, for each of the five sums,

    |sum - statement| <= SUM(n) statement,        SUM(n) = (n + 2 EXP_ULP + c) u,    c = 3 + n 2^-9

(c: 2 for the factor's roundings, 1 for the fixed remainders, n 2^-9 >= n 2^-10 + n 2^-11 for the two that grow with n).
The host forms the ratios in float64 from the device's sums, every operation correctly rounded or (log, sqrt) within an ulp:

    mass_at_position = 1 / Z          relative  SUM + 2 u
    mass_within = M / Z               relative  2 SUM + 2 u
    rms_distance = sqrt(S2 / Z)       relative  (2 SUM + 2 u) / 2 + 2 u  <=  2 SUM + 4 u  (taken)
    log_z = log Z                     absolute  SUM + 2 u |log Z|
    mean_offset = (S1_right - S1_left) / Z      absolute  (2 SUM + 4 u) (S1_left + S1_right) / Z

the last because S1_right and S1_left err by SUM of themselves, their difference rounds by u |difference| <= u (S1_left +
S1_right), and the division by Z adds SUM + u of the quotient.
"""
import numpy as np

from tests import refine_ref as rref
from tests.segment_ref import EXP_ULP, LD, QUANT_BITS, U

CUT_Q = 700 << QUANT_BITS
SUMS = ("Z", "M", "S1_left", "S1_right", "S2")


def sum_bound(n):
    """Relative bound of each of the five float64 sums over n candidates."""
    return (n + 2.0 * EXP_ULP + 3.0 + n * 2.0 ** -9) * U


def prefix(code, q_left, q_right, lo, hi):
    """[P(lo), .., P(hi)] in Python ints."""
    P = [0]
    for i in range(lo, hi):
        P.append(P[-1] + (q_left[code[i]] - q_right[code[i]] if code[i] >= 0 else 0))
    return P


def interval_one(P, lo, position, drop_q):
    """(lower, upper, n_within) of one boundary from its prefix sums."""
    need = P[position - lo] - drop_q
    inside = [lo + c for c, v in enumerate(P) if v >= need]
    return inside[0], inside[-1], len(inside)


def sums_one(P, lo, position, lower, upper):
    """(Z, M, S1_left, S1_right, S2) in longdouble, added in increasing p."""
    best = P[position - lo]
    keep = np.array([best - v <= CUT_Q for v in P])                        # the cut, compared as integers
    delta = np.array([best - v if best - v <= CUT_Q else 0 for v in P], dtype=np.float64).astype(LD)   # (exact: below 2^53)
    w = np.where(keep, np.exp(-(delta * LD(2.0 ** -QUANT_BITS))), LD(0))
    off = np.arange(len(P), dtype=np.int64) - (position - lo)              # p - p*
    in_order = lambda terms: np.cumsum(terms, dtype=LD)[-1] if len(terms) else LD(0)   # (cumsum adds one by one, in order)
    return (in_order(w), in_order(w[lower - lo:upper - lo + 1]), in_order((-off[off < 0]).astype(LD) * w[off < 0]),
            in_order(off[off > 0].astype(LD) * w[off > 0]), in_order((off * off).astype(LD) * w))


class Statement(object):
    """Of one call: position (B,), evidence (B, 3), support (B,) as tests/refine_ref.py gives them, the prefix sums per
    boundary, ``n`` (B,), and ``interval(drop_q)`` (B, 3) int64 / ``sums(drop_q)`` (B, 5) longdouble."""

    def __init__(self, sequences, k, q, seq, lo, x, hi, left_row, right_row, symbols="ATGC"):
        rows = [[int(v) for v in row] for row in np.asarray(q)]
        cache = {}
        B = len(seq)
        self.lo, self.hi = [int(v) for v in lo], [int(v) for v in hi]
        self.position, self.evidence = np.zeros(B, dtype=np.int64), np.zeros((B, 3), dtype=np.int64)
        self.support, self.P = np.zeros(B, dtype=np.int64), []
        for b in range(B):
            s = int(seq[b])
            if s not in cache:
                cache[s] = rref.codes(sequences[s], k, symbols)
            ql, qr = rows[int(left_row[b])], rows[int(right_row[b])]
            p, g, le, re, n = rref.refine_one(cache[s], ql, qr, self.lo[b], int(x[b]), self.hi[b])
            self.position[b], self.support[b], self.evidence[b] = p, n, (g, le, re)
            self.P.append(prefix(cache[s], ql, qr, self.lo[b], self.hi[b]))
            assert self.P[b][p - self.lo[b]] == le == max(self.P[b])
        self.n = np.array([h - l + 1 for l, h in zip(self.lo, self.hi)], dtype=np.int64)
        self._sums = {}

    def interval(self, drop_q):
        return np.array([interval_one(P, l, int(p), int(drop_q)) for P, l, p in zip(self.P, self.lo, self.position)],
                        dtype=np.int64).reshape(-1, 3)

    def sums(self, drop_q):
        """(B, 5) longdouble; Z, S1_left, S1_right and S2 do not depend on drop_q, M does (through lower and upper)."""
        if drop_q not in self._sums:
            iv = self.interval(drop_q)
            self._sums[drop_q] = np.array([sums_one(P, l, int(p), int(a), int(b))
                                           for P, l, p, (a, b, _) in zip(self.P, self.lo, self.position, iv)], dtype=LD).reshape(-1, 5)
        return self._sums[drop_q]


def confidence(sequences, k, q, seq, lo, x, hi, left_row, right_row, drop_q, symbols="ATGC"):
    """(position, evidence, support, interval (B, 3) int64, sums (B, 5) longdouble) of the statement."""
    st = Statement(sequences, k, q, seq, lo, x, hi, left_row, right_row, symbols)
    return st.position, st.evidence, st.support, st.interval(drop_q), st.sums(drop_q)


# ---- the behavioural case (tests/test_refine_confidence_host.py on the statement, tests/test_gpu_refine_confidence.py on the
# device) ----------------------------------------------------------------------------------------------------------------------
# A sequence of 4000 bases from two order-3 chains (tests/segment_ref.chain_sequence, as the end-to-end case of
# tests/test_gpu_refine.py builds its own) joined at base 2037; the boundary is looked for in 1000 .. 3000 around the window
# boundary 2000 with the 4-mer profiles the chains were drawn from.  The left chain is the golden reference's negative row
# 2000; the right one that row mixed with the positive row 2200: all of it ("far") or 35 % of it ("close").
# Chosen by running the statement on the CPU over the seeds 1 .. 12, drop = 3 nats: [lower, upper] holds the join for seeds
# 1 2 4 5 6 8 of the far pair and 1 2 3 4 6 7 8 9 11 of the close pair; the seeds listed are those of both.  (That half of the
# far intervals miss the join is the optimism DESIGN.md section 4.30 speaks of -- overlapping k-mers, and the three bases after
# the join drawn in the left chain's context; the tests claim no coverage.)  Statement widths upper - lower: far 29 10 16 7 22
# (median 16), close 140 870 92 162 128 (median 140).
BEHAVIOUR_SEEDS = (1, 2, 4, 6, 8)
BEHAVIOUR_MIX = {"far": 1.0, "close": 0.35}
BEHAVIOUR_LENGTH, BEHAVIOUR_JOIN, BEHAVIOUR_LO, BEHAVIOUR_X, BEHAVIOUR_HI = 4000, 2037, 1000, 2000, 3000
BEHAVIOUR_STATEMENT_WIDTHS = {"far": [29, 10, 16, 7, 22], "close": [140, 870, 92, 162, 128]}


def behaviour_case(kind, seed):
    """(sequence, log_profiles (2, 256)) of one seed of the "far" or the "close" pair."""
    from tests import compose_ref, segment_ref
    rows = compose_ref.small_rows()
    a, b = rows[0].astype(np.float64), rows[1].astype(np.float64)
    a, b = a / a.sum(), b / b.sum()
    mix = BEHAVIOUR_MIX[kind]
    left, right = a * 20000, ((1 - mix) * a + mix * b) * 20000
    seq = segment_ref.chain_sequence(np.random.default_rng(seed), [left, right], [0, BEHAVIOUR_JOIN, BEHAVIOUR_LENGTH], BEHAVIOUR_LENGTH)
    return seq, np.log(np.stack([(r + 0.5) / (r + 0.5).sum() for r in (left, right)]))


def derived(sums):
    """(log_z, mass_at_position, mass_within, mean_offset, rms_distance) in longdouble from (B, 5) sums."""
    s = np.asarray(sums, dtype=LD).reshape(-1, 5)
    Z, M, left, right, S2 = (s[:, i] for i in range(5))
    return np.log(Z), 1 / Z, M / Z, (right - left) / Z, np.sqrt(S2 / Z)


def assert_sums_within(got, want, n, what=""):
    """Every one of the (B, 5) float64 sums within SUM(n) of the statement (relative; a sum the statement has at 0 is 0)."""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1, 5), np.asarray(want, dtype=LD).reshape(-1, 5)
    bound = np.array([sum_bound(int(v)) for v in n], dtype=LD)[:, None]
    err = np.abs(got.astype(LD) - want)
    bad = np.argwhere(~(err <= bound * want))
    assert len(bad) == 0, (what, [(int(b), SUMS[c], float(got[b, c]), float(want[b, c]), float(err[b, c] / want[b, c]),
                                   float(bound[b, 0])) for b, c in bad[:6]])
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want > 0, err / np.where(want > 0, want, 1) / bound, 0)
    return float(rel.max()) if rel.size else 0.0


def assert_derived_within(conf, want_sums, n, what=""):
    """The five host-formed fields of a ``Confidence`` within their bounds of the statement's."""
    want_sums = np.asarray(want_sums, dtype=LD).reshape(-1, 5)
    log_z, at, within, mean, rms = derived(want_sums)
    sb = np.array([sum_bound(int(v)) for v in n], dtype=LD)
    spread = (want_sums[:, 2] + want_sums[:, 3]) / want_sums[:, 0]
    checks = (("log_z", conf.log_z, log_z, sb + 2 * U * np.abs(log_z)),
              ("mass_at_position", conf.mass_at_position, at, (sb + 2 * U) * at),
              ("mass_within", conf.mass_within, within, (2 * sb + 2 * U) * within),
              ("mean_offset", conf.mean_offset, mean, (2 * sb + 4 * U) * spread),
              ("rms_distance", conf.rms_distance, rms, (2 * sb + 4 * U) * rms))
    for name, got, want, bound in checks:
        err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - want)
        bad = np.flatnonzero(~(err <= bound))
        assert len(bad) == 0, (what, name, [(int(b), float(got[b]), float(want[b]), float(err[b]), float(bound[b])) for b in bad[:6]])
