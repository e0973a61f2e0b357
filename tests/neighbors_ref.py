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


# ---- helpers of tests/test_gpu_neighbors_shapes.py (pinned in tests/test_neighbors_host.py) ------------------------------
def lattice_unit(*arrays):
    """The largest power of two of which every entry of the arrays is an integer multiple (1.0 when all are zero)."""
    e = None
    for a in arrays:
        a = np.asarray(a, np.float64)
        assert np.all(np.isfinite(a))
        m, x = np.frexp(a[a != 0.0])                     # a = m 2^x, 0.5 <= |m| < 1: m 2^53 is an integer
        if m.size:
            n = np.abs(m * 2.0 ** 53).astype(np.int64)
            low = int((x + np.log2((n & -n).astype(np.float64)).astype(np.int64) - 53).min())
            e = low if e is None else min(e, low)
    return 1.0 if e is None else 2.0 ** e


def lattice_sqdist(Q, X):
    """(N, M) chain values for inputs on a lattice, by plain NumPy: with every coordinate an integer times one power of two
    u, every difference is an integer n u with |n| <= max |q - x| / u =: m (exact), every square an integer times u^2
    (exact: n^2 <= m^2 < 2^53) and every partial sum of the D squares an integer times u^2 below D m^2 u^2.  With
    D m^2 < 2^53 each of these is a float64, so neither the fma chain nor a sum in any other order ever rounds: both give
    the true value.  Asserts that precondition (u is the common unit of the inputs; |log2 u| <= 400 keeps u^2 normal)."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    assert Q.ndim == 2 and X.ndim == 2 and Q.shape[1] == X.shape[1]
    u = lattice_unit(Q, X)
    span = max(float((Q.max(axis=0) - X.min(axis=0)).max()), float((X.max(axis=0) - Q.min(axis=0)).max()), 0.0)
    assert 2.0 ** -400 <= u <= 2.0 ** 400 and Q.shape[1] * (span / u) ** 2 < 2.0 ** 53, \
        "not on a lattice coarse enough for exact sums: unit %g, max |q - x| %g, D %d" % (u, span, Q.shape[1])
    s = np.zeros((Q.shape[0], X.shape[0]))
    for c in range(Q.shape[1]):
        d = Q[:, c][:, None] - X[None, :, c]
        d *= d
        s += d
    return s


def select_by_partition(d2, k):
    """select(d2, k) without sorting whole rows: the rows at or below the k-th smallest value in ascending index, then a
    stable argsort of those few.  For rows long enough that lexsort is the cost."""
    n = d2.shape[0]
    idx = np.empty((n, k), np.int64)
    for a in range(n):
        cand = np.flatnonzero(d2[a] <= np.partition(d2[a], k - 1)[k - 1])
        idx[a] = cand[np.argsort(d2[a, cand], kind="stable")[:k]]
    return np.sqrt(np.take_along_axis(d2, idx, axis=1)), idx


def _order_statistic(d2, r):
    """The r-th smallest (1-based) entry of every row."""
    return np.partition(d2, r - 1, axis=1)[:, r - 1]


def must_fall_back(d2, k, KC):
    """(N,) bool: queries that the certificate cannot pass, from the chain values d2 (N, M) alone (masked rows +inf,
    k <= the unmasked rows).  Notation: d2_(r) the r-th smallest chain value of the query, a~ the Gram-form value of a row,
    E >= |a~ - d2| for every row, the device's list = the KC rows smallest by (a~, index), T = a~_(KC) - E with a~_(KC) the
    list's largest value, dk = the k-th smallest chain value within the list; the query is certified when every unmasked
    row is in the list or dk + 2 eps max(dk, T) < T.
    True when more than KC rows have d2 <= d2_(k): each of those KC + 1 rows has a~ <= d2_(k) + E, so the KC-th smallest
    a~ is at most d2_(k) + E and T <= d2_(k).  dk is the k-th smallest over a subset of the rows, so dk >= d2_(k) >= T, and
    dk + (something >= 0) < T fails; more than KC finite rows also rules out 'every row kept'."""
    return (d2 <= _order_statistic(d2, k)[:, None]).sum(axis=1) > KC


def must_certify(d2, E, k, KC):
    """(N,) bool: queries that the certificate has to pass, from the chain values d2 (N, M) (masked rows +inf) and the bound
    E (N,) alone; notation as in must_fall_back.  True when at most KC rows are unmasked (every row is kept), or when
    d2_(KC) - d2_(k) > 4 E.  Then:
    * the M - KC + 1 rows at or past place KC of the chain order have a~ >= d2_(KC) - E, a row of the first k has
      a~ <= d2_(k) + E < d2_(KC) - 3 E: each of the first k is below all of those, so it is among the KC - 1 smallest by a~,
      the list holds the true first k and dk = d2_(k);
    * of any KC rows one is at or past place KC, so a~_(KC) >= d2_(KC) - E and T >= d2_(KC) - 2 E > d2_(k) + 2 E = dk + 2 E;
    * eps = (D + 4) 2^-53 and E = (2 D + 64) 2^-53 s^2 with s = |q| + max |x|, and every value in play is at most
      s^2 (1 + 1e-12): 2 eps max(dk, T) < E.
    So dk + 2 eps max(dk, T) < dk + E < T with E to spare, which also covers the 1e-12 E between the host's E and the device's.
    (The gap is taken to place KC, not KC + 1: with KC rows tied at d2_(k) and a wide gap after them, a~_(KC) can fall
    below d2_(k) + E and the device rightly falls back.)  Between the two predicates -- a gap of 0 .. 4 E with at most KC
    rows at or below d2_(k) -- the route depends on the rounding of a~ and nothing is claimed."""
    n, m = d2.shape
    E = np.broadcast_to(np.asarray(E, np.float64), (n,))
    few = np.isfinite(d2).sum(axis=1) <= KC
    if m <= KC:
        return np.ones(n, bool)
    with np.errstate(invalid="ignore"):
        gap = _order_statistic(d2, KC) - _order_statistic(d2, k)          # inf - inf only where `few`
        return few | (gap > 4.0 * E)
