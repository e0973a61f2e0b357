"""Dense float64 restatement of the density scoring method (test-only): scikit-learn's
KernelDensity(kernel='gaussian', bandwidth=h).fit(X).score_samples(Q) written out with NumPy, every train row counted."""
import numpy as np


def log_density(Q, X, h):
    Q = np.asarray(Q, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    D = Q.shape[1]
    out = np.empty(Q.shape[0])
    xn = np.einsum("ij,ij->i", X, X)
    for s in range(0, Q.shape[0], 512):
        q = Q[s:s + 512]
        d2 = np.maximum(np.einsum("ij,ij->i", q, q)[:, None] + xn[None, :] - 2.0 * (q @ X.T), 0.0)
        e = -d2 / (2.0 * h * h)
        m = e.max(axis=1)
        out[s:s + 512] = m + np.log(np.exp(e - m[:, None]).sum(axis=1))
    return out - np.log(X.shape[0]) - 0.5 * D * np.log(2.0 * np.pi) - D * np.log(h)


def density_scores(Q, pos, neg, h_pos=0.005, h_neg=0.01):
    """phamer_scorer.density_score_points (scripts/phamer.py:275-287)."""
    return log_density(Q, pos, h_pos) - log_density(Q, neg, h_neg)


def close(got, want, tol):
    """|got - want| <= tol * max(1, |want|) elementwise (and the same NaN pattern)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= tol * np.maximum(1.0, np.abs(want))))
