"""NumPy / Python-integer statement of phamers_amd/compare.py, independent of the device code: the
placements by the brute-force P x N comparison, the Gram matrices in Python integers, the covariance by the rational formula,
the bootstrap by the brute-force weighted pair sum (and, for large shapes, by the run formula), the draws by the hash rule.

    placements(scores, n_pos)               -> t_pos (C, P), t_neg (C, N) int64
    grams(t_pos, t_neg)                     -> area2 (list of int), G10, G01 (object arrays of Python ints)
    placements_by_sort / grams_exact        -> the same two for shapes the P x N matrix cannot hold, entries up to 2^64
    covariance / delta / delta_variance / z / p_value
    weights(seed, b, P, N)                  -> (n,) int64: how often resample b draws each row
    bootstrap_brute / bootstrap_runs(scores, n_pos, seed, B, first=0) -> (B, C) uint64
    cells(scores, n_pos, baseline, resamples, seed, level) -> the table of compare.cells
"""
import math
from fractions import Fraction
from statistics import NormalDist

import numpy as np

MASK = (1 << 64) - 1


def splitmix64(x):
    """oracle.py's _splitmix64 on Python integers."""
    z = (x + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def _splitmix64_np(x):
    """the same on a uint64 array (arithmetic mod 2^64)."""
    with np.errstate(over='ignore'):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _mulhi64(h, n):
    """(h * n) >> 64 for a uint64 array h and 0 < n < 2^32."""
    n = np.uint64(n)
    hi, lo = h >> np.uint64(32), h & np.uint64(0xFFFFFFFF)
    return (hi * n + ((lo * n) >> np.uint64(32))) >> np.uint64(32)


def draws(seed, b, s, n_s):
    """The n_s rows (within the class) that resample b draws from class s (0 positives, 1 negatives)."""
    key = splitmix64(splitmix64(int(seed) & MASK) ^ (2 * int(b) + s))
    with np.errstate(over='ignore'):
        h = _splitmix64_np(np.uint64(key) + np.arange(n_s, dtype=np.uint64))
    return _mulhi64(h, n_s).astype(np.int64)


def weights(seed, b, P, N):
    return np.concatenate((np.bincount(draws(seed, b, 0, P), minlength=P), np.bincount(draws(seed, b, 1, N), minlength=N))).astype(np.int64)


def noisy_cells(rng, P, N, count):
    """``count`` cells for the tests: a common signal plus noise of growing width, rounded to one decimal (ties); from two
    cells on the last but one is a +-1 cell, from three on the last is an exact duplicate of cell 0."""
    base = np.r_[np.ones(P), np.zeros(N)] + rng.normal(0, 1, P + N)
    rows = [np.round(base + rng.normal(0, 0.2 * (c + 1), P + N), 1) for c in range(max(count - 2, 1))]
    if count >= 2:
        rows.append(np.where(base > 0.5, 1.0, -1.0))
    if count >= 3:
        rows.append(rows[0].copy())
    return np.array(rows)


def _matrix(scores, n_pos):
    s = np.asarray(scores, dtype=np.float64)
    if s.ndim != 2 or not 1 <= int(n_pos) < s.shape[1]:
        raise ValueError("scores must be (cells, rows) with both classes present")
    if not np.isfinite(s).all():
        raise ValueError("Input contains NaN or infinity.")
    return s, int(n_pos)


def placements(scores, n_pos):
    s, P = _matrix(scores, n_pos)
    t_pos, t_neg = [], []
    for row in s:
        x, y = row[:P, None], row[None, P:]
        k = 2 * (x > y).astype(np.int8) + (x == y)       # (P, N); -0.0 == 0.0 under NumPy's comparisons
        t_pos.append(k.sum(axis=1, dtype=np.int64))
        t_neg.append(k.sum(axis=0, dtype=np.int64))
    return np.array(t_pos, dtype=np.int64), np.array(t_neg, dtype=np.int64)


def grams(t_pos, t_neg):
    tp, tn = np.asarray(t_pos, dtype=np.int64), np.asarray(t_neg, dtype=np.int64)
    P, N = tp.shape[1], tn.shape[1]
    if 4 * N * N * P >= 2 ** 63 or 4 * P * P * N >= 2 ** 63:     # (else every sum below fits int64: t_pos <= 2 N, t_neg <= 2 P)
        tp, tn = tp.astype(object), tn.astype(object)
    return [int(v) for v in tp.sum(axis=1)], tp.dot(tp.T).astype(object), tn.dot(tn.T).astype(object)


def placements_by_sort(scores, n_pos):
    """The same without the P x N matrix, for shapes it cannot hold: with the other class sorted, #{y < x} and #{y <= x} are
    the two insertion points of x (np.searchsorted left / right), so t_pos = left + right; for a negative y among the sorted
    positives #{x > y} = P - right and #{x == y} = right - left, so t_neg = 2 P - right - left."""
    s, P = _matrix(scores, n_pos)
    t_pos, t_neg = [], []
    for row in s:
        x, y = row[:P] + 0.0, row[P:] + 0.0               # + 0.0: -0.0 -> +0.0, one value whatever the sort makes of signs
        xs, ys = np.sort(x), np.sort(y)
        t_pos.append(np.searchsorted(ys, x, side='left') + np.searchsorted(ys, x, side='right'))
        t_neg.append(2 * P - np.searchsorted(xs, y, side='right') - np.searchsorted(xs, y, side='left'))
    return np.array(t_pos, dtype=np.int64), np.array(t_neg, dtype=np.int64)


GRAM_CHUNK = 1 << 17   # rows per int64 dot product of grams_exact


def grams_exact(t_pos, t_neg):
    """``grams`` for any size the library accepts (entries below 2^64) without object arrays: int64 dot products over at
    most 2^17 rows -- placements are below 2^23 (n < 2^22 under the library's limit), so a chunk's sum stays below
    2^17 2^46 = 2^63 -- added up as Python integers."""
    out = []
    for t in (np.asarray(t_pos, dtype=np.int64), np.asarray(t_neg, dtype=np.int64)):
        if t.size and int(t.max()) >= 1 << 23:
            raise ValueError("a placement of 2^23 or more: a chunk's sum could pass int64")
        g = np.zeros((len(t), len(t)), dtype=object)
        for lo in range(0, t.shape[1], GRAM_CHUNK):
            piece = t[:, lo:lo + GRAM_CHUNK]
            g += piece.dot(piece.T).astype(object)
        out.append(g)
    area2 = [int(v) for v in np.asarray(t_pos, dtype=np.int64).sum(axis=1)]   # (<= 2 P N < 2^45)
    return area2, out[0], out[1]


class Statement(object):
    """area2, Grams and the rational covariance of one matrix (``by_sort``: placements_by_sort and grams_exact, for shapes
    the brute-force forms cannot hold)."""

    def __init__(self, scores, n_pos, by_sort=False):
        s, P = _matrix(scores, n_pos)
        self.P, self.N = P, s.shape[1] - P
        if self.P < 2 or self.N < 2:
            raise ValueError("two rows of each class")
        self.t_pos, self.t_neg = (placements_by_sort if by_sort else placements)(s, P)
        self.area2, self.G10, self.G01 = (grams_exact if by_sort else grams)(self.t_pos, self.t_neg)
        self.C = len(self.area2)

    def cov_fraction(self, a, b):
        P, N = self.P, self.N
        aa = self.area2[a] * self.area2[b]
        num10, num01 = P * int(self.G10[a][b]) - aa, N * int(self.G01[a][b]) - aa
        return Fraction(num10 * (N - 1) + num01 * (P - 1), 4 * P * P * N * N * (P - 1) * (N - 1))

    def auc(self):
        return np.array([float(Fraction(a, 2 * self.P * self.N)) for a in self.area2])

    def covariance(self):
        return np.array([[float(self.cov_fraction(a, b)) for b in range(self.C)] for a in range(self.C)]).reshape(self.C, self.C)

    def delta(self, a, b):
        return float(Fraction(self.area2[a] - self.area2[b], 2 * self.P * self.N))

    def delta_variance(self, a, b):
        return float(self.cov_fraction(a, a) + self.cov_fraction(b, b) - 2 * self.cov_fraction(a, b))

    def z(self, a, b):
        v = self.delta_variance(a, b)
        return self.delta(a, b) / math.sqrt(v) if v > 0.0 else float('nan')

    def p_value(self, a, b):
        z = self.z(a, b)
        return math.erfc(abs(z) / math.sqrt(2.0)) if z == z else float('nan')


def bootstrap_brute(scores, n_pos, seed, B, first=0):
    """area2_boot by the weighted sum over all P x N pairs."""
    s, P = _matrix(scores, n_pos)
    N = s.shape[1] - P
    kernels = [2 * (row[:P, None] > row[None, P:]).astype(np.int64) + (row[:P, None] == row[None, P:]) for row in s]
    out = np.empty((B, len(s)), dtype=np.uint64)
    for i in range(B):
        w = weights(seed, first + i, P, N)
        for c, k in enumerate(kernels):
            out[i, c] = int(w[:P].dot(k).dot(w[P:]))
    return out


def bootstrap_runs(scores, n_pos, seed, B, first=0):
    """The same by the run formula: per run of equal scores (descending) with weighted totals Wp, Wn the term is
    Wp ((N - cn_through) + (N - cn_above)), cn_above / cn_through the weighted negatives before the run / through its end."""
    s, P = _matrix(scores, n_pos)
    N = s.shape[1] - P
    orders = []
    for row in s:
        order = np.argsort(-(row + 0.0), kind='stable')
        v = row[order]
        ends = np.r_[np.flatnonzero(v[1:] != v[:-1]), len(v) - 1]
        orders.append((order, ends))
    out = np.empty((B, len(s)), dtype=np.uint64)
    for i in range(B):
        w = weights(seed, first + i, P, N)
        for c, (order, ends) in enumerate(orders):
            wo = w[order]
            cp = np.cumsum(np.where(order < P, wo, 0))[ends]
            cn = np.cumsum(np.where(order >= P, wo, 0))[ends]
            Wp, cn_above = np.diff(np.r_[0, cp]), np.r_[0, cn[:-1]]
            out[i, c] = int(np.sum(Wp * ((N - cn) + (N - cn_above))))
    return out


def boot_auc(area2_boot, P, N):
    return np.asarray(area2_boot).astype(np.float64) / float(2 * P * N)


def boot_delta(area2_boot, a, b, P, N):
    d = np.asarray(area2_boot)[:, a].astype(np.int64) - np.asarray(area2_boot)[:, b].astype(np.int64)
    return d.astype(np.float64) / float(2 * P * N)


def cells(scores, n_pos, baseline=0, resamples=2000, seed=0, level=0.95, brute=True):
    """The table of compare.cells (plus ``delta_variance`` and ``variance`` = se^2, the once-rounded forms)."""
    st = Statement(scores, n_pos)
    P, N, C = st.P, st.N, st.C
    boot = (bootstrap_brute if brute else bootstrap_runs)(scores, n_pos, seed, resamples)
    q = NormalDist().inv_cdf((1.0 + level) / 2.0)
    auc, cov = st.auc(), st.covariance()
    se = np.sqrt(np.diag(cov))
    qs = [(1.0 - level) / 2.0, (1.0 + level) / 2.0]
    bq = np.quantile(boot_auc(boot, P, N), qs, axis=0)
    bd = np.array([np.quantile(boot_delta(boot, c, baseline, P, N), qs) for c in range(C)])
    dv = np.array([st.delta_variance(c, baseline) for c in range(C)])
    return {"auc": auc, "variance": np.diag(cov).copy(), "se": se, "ci_low": auc - q * se, "ci_high": auc + q * se,
            "delta": np.array([st.delta(c, baseline) for c in range(C)]), "delta_variance": dv, "delta_se": np.sqrt(dv),
            "z": np.array([st.z(c, baseline) for c in range(C)]), "p": np.array([st.p_value(c, baseline) for c in range(C)]),
            "boot_low": bq[0], "boot_high": bq[1], "boot_delta_low": bd[:, 0], "boot_delta_high": bd[:, 1], "area2_boot": boot}
