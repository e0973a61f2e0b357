"""Dense float64 restatement of the density bandwidth sweep (test-only), built on tests/density_ref.py: the log-density at
every bandwidth, optionally leave-one-out (the self term set to -inf, the normaliser log(M - 1)), and a rank-based ROC area."""
import numpy as np

from tests import density_ref


def log_density_sweep(Q, X, hs, exclude_self=False):
    """(B, N): row b = density_ref.log_density(Q, X, hs[b]); with ``exclude_self`` query i is row i of X and pair (i, i) is
    left out by index."""
    Q = np.asarray(Q, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    if not exclude_self:
        return np.array([density_ref.log_density(Q, X, float(h)) for h in hs]).reshape(len(hs), Q.shape[0])
    assert Q.shape == X.shape and X.shape[0] > 1
    M, D = X.shape
    xn = np.einsum("ij,ij->i", X, X)
    out = np.empty((len(hs), M))
    for s in range(0, M, 512):
        q = Q[s:s + 512]
        d2 = np.maximum(np.einsum("ij,ij->i", q, q)[:, None] + xn[None, :] - 2.0 * (q @ X.T), 0.0)
        rows = np.arange(q.shape[0])
        for b, h in enumerate(hs):
            e = -d2 / (2.0 * h * h)
            e[rows, s + rows] = -np.inf
            m = e.max(axis=1)
            out[b, s:s + 512] = (m + np.log(np.exp(e - m[:, None]).sum(axis=1))
                                 - np.log(M - 1) - 0.5 * D * np.log(2.0 * np.pi) - D * np.log(h))
    return out


# ---- inputs of tests/test_gpu_density_sweep_shapes.py (pinned in tests/test_density_sweep_host.py) ----------------------
def smooth_rows(n, D, seed):
    """Normalised rows (non-negative, row sum 1) a few hundredths apart, like normalised k-mer counts: the rows of
    tests/test_gpu_density_sweep.py."""
    rng = np.random.default_rng(seed)
    base = rng.random(D) + 0.5
    x = base[None, :] * (1.0 + 0.3 * rng.standard_normal((n, D))).clip(0.05)
    return x / x.sum(axis=1, keepdims=True)


def grid_rows(D, seed):
    """(Q (130, D), X (300, D)) with every entry 0, 1/8 or 2/8, so that d^2 is an exact multiple of 1/64 however it is summed
    and equal smallest distances are the rule: data rows 170 .. 299 repeat 130 of the first 170 in another order, so most
    minima are attained twice or more, in one chunk of 256 rows or in both.  Data rows 255 and 256 are equal (a tie across
    the chunk border), so are rows 16 and 17 (inside one 16-row tile); the first 40 queries are copies of data rows, rows
    16 and 255 among them: d^2 = 0 with nothing left out."""
    rng = np.random.RandomState(seed)
    X = rng.randint(0, 3, (300, D)) / 8.0
    Q = rng.randint(0, 3, (130, D)) / 8.0
    X[170:] = X[rng.permutation(170)[:130]]
    X[256] = X[255]
    X[17] = X[16]
    Q[:40] = X[np.r_[16, 255, 7 * np.arange(2, 40)]]
    return Q, X


def near_tie_rows(D, seed):
    """(Q (130, D), X (300, D)) smooth rows in which every odd data row is its predecessor with one column moved by one
    ulp; the first 40 queries are copies of even data rows."""
    X, Q = smooth_rows(300, D, seed), smooth_rows(130, D, seed + 1)
    X[1::2] = X[0::2]
    col = (np.arange(150) * 5) % D
    X[1::2][np.arange(150), col] = np.nextafter(X[0::2][np.arange(150), col], 1.0)
    Q[:40] = X[0:80:2]
    return Q, X


def rows_at_the_minimum(Q, X, exclude_self=False):
    """(N,) how many data rows attain a query's smallest d^2 (density_ref.log_density's expression for d^2)."""
    Q, X = np.asarray(Q, dtype=np.float64), np.asarray(X, dtype=np.float64)
    d2 = np.maximum(np.einsum("ij,ij->i", Q, Q)[:, None] + np.einsum("ij,ij->i", X, X)[None, :] - 2.0 * (Q @ X.T), 0.0)
    if exclude_self:
        np.fill_diagonal(d2, np.inf)
    return (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)


def rank_auc(positive_scores, negative_scores):
    """The ROC area as the Mann-Whitney statistic: P(positive > negative) + P(equal) / 2, from mid-ranks."""
    p, n = np.asarray(positive_scores, dtype=np.float64), np.asarray(negative_scores, dtype=np.float64)
    allv = np.concatenate((p, n))
    order = np.argsort(allv, kind="mergesort")
    sv = allv[order]
    first = np.searchsorted(sv, sv, side="left")
    last = np.searchsorted(sv, sv, side="right")
    ranks = np.empty(len(allv))
    ranks[order] = 0.5 * (first + last + 1)     # mid-rank, 1-based
    u = ranks[:len(p)].sum() - len(p) * (len(p) + 1) / 2.0
    return u / (len(p) * float(len(n)))
