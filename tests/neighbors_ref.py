"""NumPy float64 restatement of the nearest-reference lookup (test-only): the squared distance is the device's chain
``acc = fma(q_c - x_c, q_c - x_c, acc)`` over the columns in order (tests.manifold_ref.fma restates the fused multiply-add
exactly), the neighbours of a query are its first k rows in order of (d2, index), the distances are sqrt(d2).
tests/test_neighbors_host.py holds it to NumPy; tests/test_gpu_neighbors.py holds the device to it, bit for bit."""
import numpy as np

from tests.manifold_ref import fma

U = 2.0 ** -53


def sqdist(Q, X):
    """(N, M) chain values of every (query, row) pair."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    s = np.zeros((Q.shape[0], X.shape[0]))
    for c in range(Q.shape[1]):
        d = Q[:, c][:, None] - X[None, :, c]
        s = fma(d, d, s)
    return s


def pair_d2(Q, X, idx):
    """(N, k) chain values of query a against the rows idx[a]."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    s = np.zeros(idx.shape)
    for c in range(Q.shape[1]):
        d = Q[:, c][:, None] - X[idx, c]
        s = fma(d, d, s)
    return s


def bound_E(Q, X):
    """The certificate's bound per query as neighbors.hip states it, from exact-enough norms: (2 D + 64) 2^-53
    (|q| + max |x|)^2."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    s = np.sqrt((Q * Q).sum(axis=1)) + np.sqrt((X * X).sum(axis=1).max())
    return (2 * Q.shape[1] + 64) * U * s * s


def select(d2, k):
    """(distances (N, k), indices (N, k) int64) of the first k entries of every row of d2 in order of (d2, index)."""
    n, m = d2.shape
    idx = np.empty((n, k), np.int64)
    for a in range(n):
        idx[a] = np.lexsort((np.arange(m), d2[a]))[:k]
    return np.sqrt(np.take_along_axis(d2, idx, axis=1)), idx


def kneighbors_ref(Q, X, k, mask=None):
    """The lookup's contract.  ``mask`` (M,) bool: rows left out; indices still point into X."""
    d2 = sqdist(Q, X)
    if mask is not None:
        d2[:, np.asarray(mask, bool)] = np.inf
    return select(d2, k)


def kneighbors_screened(Q, X, k):
    """The same result for inputs too large for the full chain (N M D emulated fused multiply-adds): the chain runs only
    on rows that can be among the first k.  With g the Gram-form squared distance in float64 and m = 1e-12 (|q| + max |x|)^2
    -- both g and the chain value lie within m / 2 of the true squared distance: their rounding errors are below
    (D + 8) 2^-52 (|q| + |x|)^2 each, 3e-14 (...)^2 at D = 256 -- every row among the first k by chain value has
    g <= g_(k) + 2 m, where g_(k) is the k-th smallest g.  The rows taken are a prefix of the order of g that holds all of
    those, the same length for every query."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    qn, xn = (Q * Q).sum(axis=1), (X * X).sum(axis=1)
    g = np.maximum(qn[:, None] + xn[None, :] - 2.0 * (Q @ X.T), 0.0)
    m = 1e-12 * (np.sqrt(qn) + np.sqrt(xn.max())) ** 2
    kth = np.partition(g, k - 1, axis=1)[:, k - 1]
    width = int((g <= (kth + 2.0 * m)[:, None]).sum(axis=1).max())
    cand = np.sort(np.argsort(g, axis=1, kind="stable")[:, :width], axis=1)      # ascending index within a query
    s = np.zeros(cand.shape)
    for c in range(Q.shape[1]):
        d = Q[:, c][:, None] - X[cand, c]
        s = fma(d, d, s)
    order = np.empty((Q.shape[0], k), np.int64)
    for a in range(Q.shape[0]):
        order[a] = np.lexsort((cand[a], s[a]))[:k]
    return np.sqrt(np.take_along_axis(s, order, axis=1)), np.take_along_axis(cand, order, axis=1)


def normalised_counts(rng, n, D, high=60):
    """n rows of random counts over their row sums (every row has counts)."""
    c = rng.integers(0, high, (n, D)).astype(np.float64)
    c[:, 0] += 1.0
    return c / c.sum(axis=1, keepdims=True)


def reference_rows(golden_dir):
    """The normalised rows of tests/golden/ref_features.npz, positive then negative, and their ids."""
    import os
    with np.load(os.path.join(golden_dir, "ref_features.npz")) as z:
        pos, neg = z["pos_counts"].astype(np.float64), z["neg_counts"].astype(np.float64)
        ids = np.concatenate((z["pos_ids"], z["neg_ids"]))
    X = np.vstack((pos, neg))
    return X / X.sum(axis=1, keepdims=True), ids, pos.shape[0]
