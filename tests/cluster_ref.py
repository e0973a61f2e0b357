"""NumPy restatement of DBSCAN and of silhouettes (test-only), with float64 direct differences.

DBSCAN, scikit-learn's dbscan_inner restated: j is a neighbour of i iff d(i, j) <= eps (i itself included); i is core iff it
has at least min_samples neighbours; the clusters are the connected components of the core points under the neighbour
relation, numbered 0, 1, ... by each component's smallest core row; a non-core point takes the smallest label among its core
neighbours, or -1.  Silhouettes: sklearn/metrics/cluster/_unsupervised.py silhouette_samples, labels encoded by np.unique."""
import numpy as np


def pair_distances(A, B):
    """(len(A), len(B)) float64 direct-difference distances."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    out = np.empty((A.shape[0], B.shape[0]))
    for i in range(A.shape[0]):
        out[i] = np.sqrt(((B - A[i]) ** 2).sum(axis=1))
    return out


def eps_margin(X, eps):
    """min |d_ij - eps| over all pairs i < j."""
    X = np.asarray(X, dtype=np.float64)
    m = np.inf
    for s in range(0, X.shape[0], 256):
        d = pair_distances(X[s:s + 256], X)
        iu = np.arange(s, min(s + 256, X.shape[0]))[:, None] < np.arange(X.shape[0])[None, :]
        if iu.any():
            m = min(m, float(np.abs(d[iu] - eps).min()))
    return m


def dbscan(X, eps, min_samples):
    """(labels int64, core mask bool)."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    nbr = [None] * n
    for s in range(0, n, 256):
        d = pair_distances(X[s:s + 256], X)
        for r in range(d.shape[0]):
            nbr[s + r] = np.flatnonzero(d[r] <= eps)
    core = np.array([len(v) >= min_samples for v in nbr], dtype=bool)
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in np.flatnonzero(core):
        for j in nbr[i]:
            if core[j]:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    labels = np.full(n, -1, dtype=np.int64)
    k = 0
    for i in np.flatnonzero(core):       # rows in order: a component's root (its smallest core row) comes first
        r = find(i)
        if r == i:
            labels[i] = k
            k += 1
        else:
            labels[i] = labels[r]
    for i in np.flatnonzero(~core):
        c = [labels[j] for j in nbr[i] if core[j]]
        if c:
            labels[i] = min(c)
    return labels, core


def dbscan_cells(X, eps, min_samples):
    """dbscan() for D <= 3 at any size: rows hashed into cells of side eps, neighbours searched in the 3^D cells around a
    row's own; the same float64 direct-difference test d(i, j) <= eps and the same labelling rules.  (labels, core)."""
    X = np.asarray(X, dtype=np.float64)
    n, D = X.shape
    assert D <= 3
    cell = np.floor(X / eps).astype(np.int64)
    cell -= cell.min(axis=0) - 1
    span = cell.max(axis=0) + 2
    key = np.zeros(n, dtype=np.int64)
    for k in range(D):
        key = key * span[k] + cell[:, k]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    offsets = [0]
    for k in range(D):
        offsets = [o * span[k] + d for o in offsets for d in (-1, 0, 1)]
    # candidate pairs (i, j) of neighbouring cells, all at once per offset
    ii, jj = [], []
    for o in offsets:
        lo = np.searchsorted(skey, key + o, side="left")
        hi = np.searchsorted(skey, key + o, side="right")
        cnt = hi - lo
        i = np.repeat(np.arange(n), cnt)
        start = np.repeat(lo - np.cumsum(cnt) + cnt, cnt)
        j = order[start + np.arange(cnt.sum())]
        ii.append(i)
        jj.append(j)
    i, j = np.concatenate(ii), np.concatenate(jj)
    d = np.sqrt(((X[i] - X[j]) ** 2).sum(axis=1))
    nb = d <= eps
    i, j = i[nb], j[nb]
    core = np.bincount(i, minlength=n) >= min_samples
    # components of the core graph: union-find with the smaller root kept
    parent = np.arange(n)
    cc = core[i] & core[j]
    a, b = i[cc], j[cc]
    while True:
        ra, rb = parent[a], parent[b]
        lo_, hi_ = np.minimum(ra, rb), np.maximum(ra, rb)
        if (lo_ == hi_).all():
            break
        np.minimum.at(parent, hi_, lo_)
        while True:                                   # pointer jumping to the roots
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    labels = np.full(n, -1, dtype=np.int64)
    roots = parent[core]
    uniq = np.unique(roots)                           # a root is its component's smallest core row: row order = label order
    labels[core] = np.searchsorted(uniq, roots)
    bd = ~core[i] & core[j]                           # border points: the smallest label of their core neighbours
    lab = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(lab, i[bd], labels[j[bd]])
    has = ~core & (lab != np.iinfo(np.int64).max)
    labels[has] = lab[has]
    return labels, core


def silhouettes(X, labels):
    n = np.asarray(X).shape[0]
    return np.concatenate([silhouettes_sample(X, labels, np.arange(s, min(s + 256, n))) for s in range(0, n, 256)])


def silhouettes_sample(X, labels, rows):
    """silhouettes of the given rows only (the whole data set as the clusters)."""
    X = np.asarray(X, dtype=np.float64)
    _, lab = np.unique(np.asarray(labels), return_inverse=True)
    lab = lab.ravel()
    K = int(lab.max()) + 1
    if not 2 <= K <= X.shape[0] - 1:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % K)
    freq = np.bincount(lab, minlength=K)
    rows = np.asarray(rows)
    d = pair_distances(X[rows], X)
    sums = np.stack([np.bincount(lab, weights=row, minlength=K) for row in d])
    own = lab[rows]
    r = np.arange(len(rows))
    with np.errstate(divide="ignore", invalid="ignore"):
        a = sums[r, own] / (freq[own] - 1)
        other = sums / freq
        other[r, own] = np.inf
        b = other.min(axis=1)
        return np.nan_to_num((b - a) / np.maximum(a, b))


def sort_assignment_by_size(assignment, ascending=True):
    """scripts/learning.py:166-182: clusters relabelled 0.. in the order of sorted(zip(sizes, clusters)), reversed when not
    ascending; -1 stays -1."""
    assignment = np.asarray(assignment)
    clusters = sorted(set(assignment.tolist()) - {-1})
    order = sorted(zip([int(np.sum(assignment == c)) for c in clusters], clusters))
    if not ascending:
        order = order[::-1]
    out = np.full(len(assignment), -1, dtype=int)
    for new, (_, c) in enumerate(order):
        out[assignment == c] = new
    return out


def border_tie(order):
    """Two clusters of four points on a line and one point between them, within eps = 0.9 of one core point of each and
    not core itself (3 neighbours < min_samples = 4): it takes the smaller of the two labels, which the row order decides.
    ``order``: the parts 'a', 'b' (the clusters) and 'p' (the point) in row order."""
    a = np.array([[0.0, 0.0], [0.1, 0.0], [0.2, 0.0], [0.3, 0.0]])
    parts = {'a': a, 'b': a + [2.0, 0.0], 'p': np.array([[1.15, 0.0]])}
    return np.vstack([parts[c] for c in order])
