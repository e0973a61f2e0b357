"""NumPy float64 statement of a cell of the k_neighbors x k_clusters grid (test-only; phamers_amd/combo_grid.py, DESIGN.md
4.18): chain values by tests.neighbors_ref.sqdist with the rows of the query's own fold at +inf, neighbours in order of
(chain value, index into vstack(positive, negative)), the vote of every k from the rank-ordered class bits (an even split
is -1), and the k-means half tanh((en - ep) / (ep + en)) of the square roots of the smallest chain values to given
centroids.  tests/test_combo_grid_host.py holds it to scikit-learn, the oracle and a plain Python brute force;
tests/test_gpu_combo_grid.py and tests/test_gpu_combo_grid_shapes.py hold the device to it."""
import numpy as np

from tests import neighbors_ref


def blob_rows(seed, n, D=20):
    """The blob fixture: six centres in D columns, rows cycling through them with a little noise."""
    rng = np.random.RandomState(seed)
    c = rng.rand(6, D)
    return c[np.arange(n) % 6] + 0.02 * rng.randn(n, D)


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


def word_fixture():
    """(X, fold_of, is_pos) for the neighbour word at its full width (tests/test_gpu_combo_grid_shapes.py): 200 rows in 17
    columns, the classes alternating and 0.35 apart in every column, three folds with train sets of 130 rows and more.
    tests/test_combo_grid_host.py pins what the statement says of it: even splits at k = 64, rows that vote differently at
    63 and 64, both values of bit 63."""
    rng = np.random.RandomState(11)
    M, D = 200, 17
    is_pos = np.arange(M) % 2 == 0
    X = rng.randn(M, D) + 0.35 * is_pos[:, None]
    fold_of = np.arange(M) * 7 % 3
    fold_of[:5] = 0
    return X, fold_of.astype(np.int64), is_pos


def edge_folds(M):
    """Four fold ids for M >= 8 rows: fold 2 holds nothing, fold 3 the single row M // 2, fold 1 every third row and
    fold 0 the rest (about two thirds)."""
    fold_of = np.where(np.arange(M) % 3 == 0, 1, 0).astype(np.int64)
    fold_of[M // 2] = 3
    return fold_of


def tie_rows(M):
    """(X, is_pos): the rows of tie_fixture, positive then negative, repeated to M rows."""
    P, N = tie_fixture()
    at = np.arange(M) % (len(P) + len(N))
    return np.vstack((P, N))[at], at < len(P)


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


def kmeans_scores_for(X, fold_of, centroids):
    """kmeans_scores for fold ids of the caller's own (any ids, a fold may hold no row): ``centroids[fold]`` = (positive
    centroids, negative centroids); a row of a fold that is not a key stays NaN."""
    X, fold_of = np.asarray(X, np.float64), np.asarray(fold_of)
    out = np.full(len(X), np.nan)
    for f, (cp, cn) in centroids.items():
        rows = np.flatnonzero(fold_of == f)
        if rows.size == 0:
            continue
        ep = np.sqrt(neighbors_ref.sqdist(X[rows], cp).min(axis=1))
        en = np.sqrt(neighbors_ref.sqdist(X[rows], cn).min(axis=1))
        out[rows] = np.tanh((en - ep) / (ep + en))
    return out
