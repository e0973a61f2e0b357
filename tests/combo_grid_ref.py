"""NumPy float64 statement of a cell of the k_neighbors x k_clusters grid (test-only; phamers_amd/combo_grid.py, DESIGN.md
4.18): chain values by tests.neighbors_ref.sqdist with the rows of the query's own fold at +inf, neighbours in order of
(chain value, index into vstack(positive, negative)), the vote of every k from the rank-ordered class bits (an even split
is -1), and the k-means half tanh((en - ep) / (ep + en)) of the square roots of the smallest chain values to given
centroids.  tests/test_combo_grid_host.py holds it to scikit-learn and the oracle; tests/test_gpu_combo_grid.py holds the
device to it."""
import numpy as np

from tests import neighbors_ref


def blob_rows(seed, n):
    """The blob fixture: six centres in 20 columns, rows cycling through them with a little noise."""
    rng = np.random.RandomState(seed)
    c = rng.rand(6, 20)
    return c[np.arange(n) % 6] + 0.02 * rng.randn(n, 20)


def blob_fixture():
    return blob_rows(1, 70), blob_rows(2, 75)


def tie_fixture():
    """Integer-valued rows (D = 8, entries 0..3, 40 + 40) with duplicates across the classes, across folds and inside one
    fold (which pairs share a fold depends on the plan: the test checks that all three kinds occur)."""
    rng = np.random.RandomState(7)
    P = rng.randint(0, 4, (40, 8)).astype(np.float64)
    N = rng.randint(0, 4, (40, 8)).astype(np.float64)
    N[:12] = P[:12]            # across the classes
    P[20:30] = P[10:20]        # inside the positive class
    N[25:35] = N[15:25]        # inside the negative class
    P[30:34] = P[0]            # one row five times
    return P, N


def fold_ids(n_pos, n_neg, folds, seed):
    from phamers_amd.cross_validate import FoldPlan
    plan = FoldPlan(n_pos, n_neg, folds, seed)
    return np.concatenate((plan.positive, plan.negative)).astype(np.int64)


def neighbour_bits(X, fold_of, is_pos, kmax):
    """(M, kmax) bool: the class of every row's first kmax neighbours outside its own fold, in rank order."""
    d2 = neighbors_ref.sqdist(X, X)
    d2[fold_of[:, None] == fold_of[None, :]] = np.inf
    _, idx = neighbors_ref.select(d2, kmax)
    return np.asarray(is_pos, bool)[idx]


def votes(bits, k):
    v = bits[:, :k].sum(axis=1)
    return np.where(2 * v > k, 1.0, -1.0)


def knn_scores(P, N, folds, seed, ks):
    X = np.vstack((P, N))
    fold_of = fold_ids(len(P), len(N), folds, seed)
    is_pos = np.r_[np.ones(len(P), bool), np.zeros(len(N), bool)]
    bits = neighbour_bits(X, fold_of, is_pos, max(ks))
    return np.array([votes(bits, k) for k in ks])


def kmeans_scores(P, N, folds, seed, centroids):
    """``centroids[fold]`` = (positive centroids, negative centroids): the k-means half of every row's score."""
    X = np.vstack((P, N))
    fold_of = fold_ids(len(P), len(N), folds, seed)
    out = np.empty(len(X))
    for f in range(folds):
        rows = np.flatnonzero(fold_of == f)
        if rows.size == 0:
            continue
        ep = np.sqrt(neighbors_ref.sqdist(X[rows], centroids[f][0]).min(axis=1))
        en = np.sqrt(neighbors_ref.sqdist(X[rows], centroids[f][1]).min(axis=1))
        out[rows] = np.tanh((en - ep) / (ep + en))
    return out
