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
