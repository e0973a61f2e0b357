"""NumPy restatement of learning.dbscan_sweep (test-only): tests/cluster_ref.dbscan once per cell of the grid, in the order
``for eps in eps_values: for m in min_samples_values``, and the summary numbers of every cell.  Below that the inputs of
tests/test_gpu_dbscan_sweep_shapes.py and the conditions those inputs have to meet, which tests/test_dbscan_sweep_host.py
asserts without a device."""
import math

import numpy as np

from tests import cluster_ref

SUMMARY = ("n_clusters", "n_core", "n_border", "n_noise", "largest")


def summarize(labels, core):
    """The summary numbers of one cell from its labels (-1 = noise) and its core mask."""
    labels = np.asarray(labels)
    core = np.asarray(core, dtype=bool)
    clustered = labels >= 0
    sizes = np.bincount(labels[clustered]) if clustered.any() else np.zeros(1, dtype=int)
    return {"n_clusters": int(len(set(labels[clustered].tolist()))), "n_core": int(core.sum()),
            "n_border": int((clustered & ~core).sum()), "n_noise": int((~clustered).sum()), "largest": int(sizes.max())}


def dbscan_sweep(X, eps_values, min_samples_values):
    """One record per cell: eps, min_samples, labels (int64), core_sample_indices and the summary numbers."""
    records = []
    for eps in eps_values:
        for m in min_samples_values:
            labels, core = cluster_ref.dbscan(X, float(eps), int(m))
            record = {"eps": float(eps), "min_samples": int(m), "labels": labels, "core_sample_indices": np.flatnonzero(core)}
            record.update(summarize(labels, core))
            records.append(record)
    return records


def same_records(got, want, keys=("eps", "min_samples", "labels", "core_sample_indices") + SUMMARY):
    """assert that two lists of records agree in every key of ``keys`` (arrays by array_equal)."""
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        for key in keys:
            if isinstance(w[key], np.ndarray) or isinstance(g[key], np.ndarray):
                assert np.asarray(g[key]).dtype.kind == np.asarray(w[key]).dtype.kind, (i, key)
                assert np.array_equal(g[key], w[key]), (i, key, g["eps"], g["min_samples"])
            else:
                assert g[key] == w[key], (i, key, g[key], w[key])


# ---- inputs and preconditions of tests/test_gpu_dbscan_sweep_shapes.py -----------------------------------------------------
TILE = 64                                   # pair_tile.h's CL_T
LATTICE_EPS = (0.75, 1.5, 0.5, 1.0)         # unsorted on purpose; each is the distance of hundreds of lattice pairs


def groups(cus, qblocks, tiles):
    """cluster.hip's cl_groups restated: workgroups per query block, ceil(8 cus / qblocks) but at least 1 and at most tiles."""
    want = 8 * int(cus)
    g = 1 if qblocks >= want else -(-want // int(qblocks))
    return max(1, min(g, int(tiles)))


def group_tiles(T, G):
    """The tiles each of the G column groups walks: [T b / G, T (b + 1) / G)."""
    return [T * (b + 1) // G - T * b // G for b in range(G)]


def lattice_tiles(cus):
    """T = 2 isqrt(8 cus) tiles a side: T^2 is about four times the 8 cus workgroups at which every group is one tile."""
    return 2 * math.isqrt(8 * int(cus))


def lattice_rows(cus):
    return TILE * lattice_tiles(cus) - 23


def scattered_lattice(n, seed):
    """(n, 2) rows on the lattice of quarters: half of them uniform on a square of side int(3.1 sqrt(n)) lattice steps, the
    other half within 6 steps of 12 lattice centres, all permuted.  Every squared distance is exact in float64."""
    rng = np.random.RandomState(seed)
    side = int(3.1 * np.sqrt(n))
    half = n // 2
    uniform = 0.25 * rng.randint(0, side, (half, 2))
    centres = 0.25 * rng.randint(0, side, (12, 2))
    dense = centres[rng.randint(0, 12, n - half)] + 0.25 * rng.randint(-6, 7, (n - half, 2))
    X = np.vstack([uniform, dense])[rng.permutation(n)]
    assert_dyadic(X)
    return X


def assert_dyadic(X):
    """Multiples of 1/4 below 2^10 in size: a squared distance is a multiple of 1/16 below D 2^22, exact in any order."""
    X = np.asarray(X)
    assert np.array_equal(X * 4, np.round(X * 4)) and np.abs(X).max() < 2.0 ** 10


def pairs_exactly_at(X, eps_values):
    """Per eps the number of pairs i < j of 2-D dyadic rows with d_ij == eps, counted in integers: the rows as a histogram
    over the lattice, and per lattice offset (dx, dy) with dx^2 + dy^2 = 16 eps^2 the histogram against itself shifted."""
    Z = np.round(np.asarray(X) * 4).astype(np.int64)
    assert Z.shape[1] == 2
    Z -= Z.min(axis=0)
    H = np.zeros(tuple(Z.max(axis=0) + 1), dtype=np.int64)
    np.add.at(H, (Z[:, 0], Z[:, 1]), 1)
    counts = []
    for eps in eps_values:
        w = int(round(16 * eps * eps))
        assert w == 16 * eps * eps and w > 0
        r = math.isqrt(w)
        ordered = 0
        for dx in range(-r, r + 1):
            dy = math.isqrt(w - dx * dx)
            if dy * dy != w - dx * dx or dx < 0 or abs(dx) >= H.shape[0] or dy >= H.shape[1]:
                continue
            for sy in ((dy, -dy) if dx and dy else (dy,)):             # offsets with dx > 0, or dx = 0 and dy > 0: i < j once
                A = H[:H.shape[0] - dx] if dx else H
                B = H[dx:]
                ordered += int((A[:, :H.shape[1] - dy] * B[:, dy:]).sum()) if sy >= 0 else int((A[:, dy:] * B[:, :H.shape[1] - dy]).sum())
        counts.append(ordered)
    return counts


def sweep_cells(X, cells):
    """One record per (eps, min_samples) pair of ``cells``, in their order: cluster_ref.dbscan_cells for D <= 3 (any n),
    cluster_ref.dbscan otherwise."""
    X = np.asarray(X, dtype=np.float64)
    fit = cluster_ref.dbscan_cells if X.shape[1] <= 3 else cluster_ref.dbscan
    records = []
    for eps, m in cells:
        labels, core = fit(X, float(eps), int(m))
        record = {"eps": float(eps), "min_samples": int(m), "labels": labels, "core_sample_indices": np.flatnonzero(core)}
        record.update(summarize(labels, core))
        records.append(record)
    return records


def records_of_run(out, cells):
    """_lib.DbscanRows.run's output as records like sweep_cells', every number from the labels and the core mask except
    n_clusters, which is the library's own."""
    records = []
    for c, (eps, m) in enumerate(cells):
        labels = out["labels"][c].astype(np.int64)
        core = (out["coremask"] >> np.uint64(c)) & np.uint64(1) != 0
        record = {"eps": float(eps), "min_samples": int(m), "labels": labels, "core_sample_indices": np.flatnonzero(core)}
        record.update(summarize(labels, core))
        assert record["n_clusters"] == labels.max() + 1                       # labels are 0 .. K - 1, none left out
        record["n_clusters"] = int(out["n_clusters"][c])
        records.append(record)
    return records


def core_somewhere(records, n):
    """(nu, nb): the rows that are core in some cell, and the rows that are not core in some cell."""
    times = np.zeros(n, dtype=np.int64)
    for r in records:
        times[r["core_sample_indices"]] += 1
    return int(np.count_nonzero(times > 0)), int(np.count_nonzero(times < len(records)))


def borders_between_clusters(X, record):
    """The number of border rows of the cell whose core neighbours carry more than one label."""
    X = np.asarray(X, dtype=np.float64)
    labels = record["labels"]
    core = np.zeros(len(X), dtype=bool)
    core[record["core_sample_indices"]] = True
    border = np.flatnonzero(~core & (labels >= 0))
    cores = np.flatnonzero(core)
    count = 0
    for s in range(0, len(border), 256):
        near = cluster_ref.pair_distances(X[border[s:s + 256]], X[cores]) <= record["eps"]
        for row in near:
            count += len(set(labels[cores[row]].tolist())) > 1
    return count


def clumps(n=150, D=3, seed=64):
    """Dyadic rows around 5 lattice centres: the rows of the threshold-table cases."""
    rng = np.random.RandomState(seed)
    centres = 0.25 * rng.randint(0, 40, (5, D))
    X = centres[rng.randint(0, 5, n)] + 0.25 * rng.randint(-5, 6, (n, D))
    assert_dyadic(X)
    return X


CLUMP_MIN_SAMPLES = (1, 2, 3, 4, 6, 9, None, 2 ** 40)          # None: n + 1


def clump_cells(X, seed=64, count=64):
    """``count`` cells, every one on a threshold of its own: the smallest distinct non-zero pair distances of X (float64
    square roots of exact sums, most of them irrational: the pair AT the threshold is a neighbour only if the device's
    threshold is the right double), shuffled, each with a min_samples drawn from CLUMP_MIN_SAMPLES."""
    rng = np.random.RandomState(seed + 1)
    d = cluster_ref.pair_distances(X, X)
    eps = np.unique(d[d > 0])[:count]
    assert len(eps) == count
    eps = eps[rng.permutation(count)]
    ms = [CLUMP_MIN_SAMPLES[k] for k in rng.randint(0, len(CLUMP_MIN_SAMPLES), count)]
    return [(float(e), len(X) + 1 if m is None else m) for e, m in zip(eps, ms)]


def cells_64(cells, thresholds):
    """64 cells on the first ``thresholds`` eps values of ``cells`` (in their shuffled order), 64 / thresholds min_samples
    values each, interleaved: consecutive cells differ in eps, and a threshold's cells are spread over the 64."""
    eps = [e for e, _ in cells[:thresholds]]
    per = 64 // thresholds
    ms = ([3, 6, 1, 2, 4, 9, 5, 7, 8] + list(range(10, 33)))[:per]
    out = [(eps[(5 * c) % thresholds], ms[(c + c // thresholds) % per]) for c in range(64)]
    assert len(set(out)) == 64 and len({e for e, _ in out}) == thresholds and len({m for _, m in out}) == per
    assert all(a[0] != b[0] for a, b in zip(out, out[1:]))
    return out


def bin_counts(X, eps_values):
    """Pairs i != j of dyadic X per bin of the sorted distinct eps values: counts[b] = pairs with exactly b thresholds below
    their distance, b = 0 .. E (E: beyond the largest).  Decided on the exact squared distances."""
    d = cluster_ref.pair_distances(X, X)
    d = d[~np.eye(len(X), dtype=bool)]
    th = np.unique(np.asarray(eps_values, dtype=np.float64))
    return np.bincount(np.searchsorted(th, d, side="left"), minlength=len(th) + 1)


def blobs(n, D, seed):
    """Four Gaussian blobs and a tenth of the rows displaced (tests/test_gpu_dbscan_sweep.py's _blobs)."""
    rng = np.random.RandomState(seed)
    centres = 3.0 * rng.randn(4, D)
    X = centres[rng.randint(0, 4, n)] + 0.35 * rng.randn(n, D)
    X[rng.rand(n) < 0.1] += 2.0 * rng.randn(D)
    return X


MARGIN = 2.0 ** -40       # relative; the device's fma chain is within about (D + 3) 2^-53 of s, 2^-46 at D = 100


def extended_distances(X):
    """(n, n) np.longdouble direct-difference distances (64-bit significand: asserted)."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    X = np.asarray(X, dtype=np.float64).astype(np.longdouble)
    out = np.empty((len(X), len(X)), dtype=np.longdouble)
    for i in range(len(X)):
        out[i] = np.sqrt(((X - X[i]) ** 2).sum(axis=1))
    return out


def midpoint_eps(d, quantiles=(0.02, 0.05, 0.1, 0.2)):
    """float64 eps values midway between two consecutive sorted pair distances, at the given quantiles of the pairs."""
    v = np.sort(d[np.triu_indices(len(d), 1)])
    return [float((v[int(q * len(v))] + v[int(q * len(v)) + 1]) / 2) for q in quantiles]


def relative_margin(d, eps_values):
    """min over pairs i < j and eps of |d_ij - eps| / eps."""
    v = d[np.triu_indices(len(d), 1)]
    return float(min(np.abs(v - np.longdouble(e)).min() / np.longdouble(e) for e in eps_values))


def dbscan_of_distances(d, eps, min_samples):
    """cluster_ref.dbscan's rules on a given matrix of distances (any float type; NaN is no neighbour): (labels, core)."""
    n = len(d)
    near = d <= eps
    core = near.sum(axis=1) >= min_samples
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in np.flatnonzero(core):
        for j in np.flatnonzero(near[i] & core):
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    labels = np.full(n, -1, dtype=np.int64)
    k = 0
    for i in np.flatnonzero(core):
        r = find(i)
        if r == i:
            labels[i] = k
            k += 1
        else:
            labels[i] = labels[r]
    for i in np.flatnonzero(~core):
        c = labels[np.flatnonzero(near[i] & core)]
        if len(c):
            labels[i] = c.min()
    return labels, core


def cells_of_distances(d, cells):
    records = []
    for eps, m in cells:
        labels, core = dbscan_of_distances(d, eps, int(m))
        record = {"eps": float(eps), "min_samples": int(m), "labels": labels, "core_sample_indices": np.flatnonzero(core)}
        record.update(summarize(labels, core))
        records.append(record)
    return records


def rows_with_infinities(seed=7):
    """100 finite rows (D = 4, three blobs) and 7 rows holding +-inf scattered among them: distances to and between those
    rows are +inf or NaN (inf - inf), never <= eps.  Returns (X, the indices of the 7 rows)."""
    rng = np.random.RandomState(seed)
    centres = np.array([[0.0, 0.0, 0.0, 0.0], [2.0, 1.0, 0.0, -1.0], [-1.0, 3.0, 1.0, 0.5]])
    X = centres[rng.randint(0, 3, 107)] + 0.3 * rng.randn(107, 4)
    where = np.sort(rng.choice(107, 7, replace=False))
    inf = np.inf
    X[where[0], 0] = inf
    X[where[1], 0] = inf                    # the same column as the row before: their distance is NaN
    X[where[2], 0] = -inf
    X[where[3], 3] = inf
    X[where[4], [1, 2]] = [inf, -inf]
    X[where[5]] = inf
    X[where[6]] = X[where[0]]               # a copy of an infinite row: NaN to it and to itself
    return X, where
