"""
learning.py -- drop-in for the hot-path helpers of PhaMers' scripts/learning.py.

    knn(queries, ref_data, ref_labels, k=3)       scripts/learning.py:118-128   -> GPU
    distances(vector, data)                       scripts/learning.py:47-56     -> GPU (float64, direct differences)
    closest_to(point, picks)                      scripts/learning.py:59-66     -> GPU distances + first-index argmin
    kmeans(data, k, ...)                          scripts/learning.py:131-146   -> scikit-learn's seeding on the host + its Lloyd sweeps on the GPU
    get_centroids(data, assignment)               scripts/learning.py:69-81     -> NumPy (86 means)
    get_density(point, data, bandwidth=0.1)       scripts/learning.py:107-115   -> GPU (float64 Gaussian KDE, log_density batched)
    density_sweep(queries, data, bandwidths)      (the choice of the density bandwidths) -> GPU, every bandwidth from one pass over the pairs (phk_kde_sweep)
    dbscan(data, eps, min_samples, ...)           scripts/learning.py:149-163   -> GPU (neighbour counts + lock-free union-find)
    dbscan_sweep(data, eps_values, min_samples_values)   (the choice of dbscan's parameters) -> GPU, every cell of the grid in one pass over the pairs (phk_dbscan_sweep)
    kdistances(data, k)                           (the k-distance curve)        -> GPU kneighbors, sorted k-th distances
    silhouettes(data, assignment)                 scripts/learning.py:84-92     -> GPU (float64 cluster distance sums)
    cluster_silhouettes(data, assignment, c)      scripts/learning.py:95-104    -> GPU silhouettes of one cluster's members
    place_contigs(reference, contigs, k)          scripts/analysis.py:771-776   -> GPU, all contigs as one batch (phk_placement_run)
    kmeans_sweep(data, k_values, seeds)           scripts/cluster.py:38-47      -> GPU, all (k, seed) fits as one batch (phk_sweep_run)
    silhouette_score(data, labels)                (sklearn.metrics name)        -> mean of the GPU silhouettes
    cluster_deviations(data, assignment)          scripts/learning.py:31-44     -> NumPy (O(n D))
    sort_assignment_by_size(assignment, ...)      scripts/learning.py:166-182   -> NumPy

k-means reproduces the reference's scikit-learn fit (a per-run fit that does not depend on the number of
query contigs; the golden scores are pinned to its centroids): the k-means++
seeding is scikit-learn's own, on the host, the Lloyd iteration runs on the device (phk_kmeans_lloyd) and
gives the same labels; PHAMERS_KMEANS=sklearn keeps the whole fit on the host, PHAMERS_KMEANS=gpu selects
kmeans_gpu, a deterministic, version-independent device k-means (phk_kmeans).
"""
import logging

import numpy as np

from . import _lib

kmeans_seed = 10  # scripts/learning.py:21

logging.basicConfig(format='[%(asctime)s][%(levelname)s][%(funcName)s] - %(message)s')
logger = logging.getLogger(__name__)
logger.setLevel(logging.WARNING)


def knn(queries, ref_data, ref_labels, k=3):
    """K-nearest-neighbours vote (scripts/learning.py:118-128): Euclidean, uniform weights,
    labels in {0, 1}; returns 2*(predicted label - 0.5), i.e. -1.0 / +1.0 per query."""
    ref_data = np.asarray(ref_data, dtype=np.float64)
    labels = np.asarray(ref_labels)
    if not np.all((labels == 0) | (labels == 1)):
        raise NotImplementedError("phamers_amd.learning.knn handles the reference's {0,1} labels only")
    queries = np.asarray(queries, dtype=np.float64)
    if np.isnan(queries).any() or np.isnan(ref_data).any():
        raise ValueError("Input contains NaN.")  # what scikit-learn raises for the reference
    ctx = _lib.get_context()
    model = _lib.Model(ctx, ref_data[labels == 1], ref_data[labels == 0], k_neighbors=k)
    try:
        return model.score(queries, "knn")
    finally:
        model.close()


def distances(vector, data):
    """Distances from one point to many (scripts/learning.py:47-56): ``vector`` (D,) or (1, D), ``data`` (M, D) ->
    (M,) float64, sqrt of the direct-difference sums, computed on the device (phk_distances).  Any other ``vector``
    shape fails to broadcast in the reference's ``np.repeat(vector, M, axis=0) - data`` and raises here as well."""
    vector = np.asarray(vector, dtype=np.float64)
    data = np.ascontiguousarray(data, dtype=np.float64)
    if vector.ndim == 1:
        vector = vector[None, :]
    if vector.shape[0] != 1:
        # np.repeat(vector, M, axis=0) - data only broadcasts for one row; anything else raises in the reference too
        raise ValueError("operands could not be broadcast together with shapes %s %s"
                         % ((vector.shape[0] * data.shape[0], vector.shape[1]), data.shape))
    if vector.shape[1] != data.shape[1]:
        raise ValueError("operands could not be broadcast together with shapes %s %s"
                         % ((data.shape[0], vector.shape[1]), data.shape))
    out = np.empty((1, data.shape[0]), dtype=np.float64)
    ctx = _lib.get_context()
    _lib.check(ctx.lib.phk_distances(ctx.handle, _lib.ptr(np.ascontiguousarray(vector)), 1, _lib.ptr(data),
                                     data.shape[0], data.shape[1], _lib.ptr(out)))
    return out[0]


def kneighbors(queries, data, k=5, _batch_rows=0, _details=None):
    """The k nearest rows of ``data`` (M, D) for every row of ``queries`` (N, D): ``(distances, indices)`` as scikit-learn's
    NearestNeighbors(n_neighbors=k, algorithm='brute').fit(data).kneighbors(queries) orders them, (N, k) float64 and (N, k)
    int64.  The distances are the numbers ``distances`` returns (sqrt of the direct-difference sums accumulated in column
    order); equal distances are ordered by index.  1 <= k <= 28.  Computed on the device (phk_neighbors): a float64 MFMA
    proposal, an exact refinement, a certificate and an exact fallback -- the result does not depend on the route.
    ``_batch_rows`` / ``_details`` are for the tests: queries per batch, and a dict that receives ``fell_back``, ``queries``,
    the per-query bound ``E`` and the Gram-form ``approx_d2`` of the returned neighbours."""
    queries = np.asarray(queries, dtype=np.float64)
    data = np.asarray(data, dtype=np.float64)
    _lib.check_neighbor_arguments(queries, data, k)
    if np.isnan(queries).any() or np.isnan(data).any():
        raise ValueError("Input contains NaN.")
    return _lib.neighbors(_lib.get_context(), queries, data, k, _batch_rows, _details)


def closest_to(point, picks):
    """The row of ``picks`` closest to ``point`` (scripts/learning.py:59-66): first index wins ties, as np.argmin."""
    picks = np.asarray(picks)
    return picks[np.argmin(distances(point, picks))]


def kmeans_gpu(data, k, seed=kmeans_seed, max_iter=300):
    """Deterministic device k-means (phk_kmeans): (labels, centroids, sweeps).  Version independent and
    bit-reproducible; NOT the scikit-learn result the reference's scores are pinned to."""
    import ctypes
    X = np.ascontiguousarray(data, dtype=np.float64)
    n, D = X.shape
    centroids = np.empty((k, D), dtype=np.float64)
    labels = np.empty(n, dtype=np.uint32)
    n_iter = ctypes.c_int()
    ctx = _lib.get_context()
    _lib.check(ctx.lib.phk_kmeans(ctx.handle, _lib.ptr(X), n, D, int(k), int(seed), int(max_iter), _lib.ptr(centroids),
                                  _lib.ptr(labels), ctypes.byref(n_iter)))
    return labels.astype(np.int64), centroids, n_iter.value


def kmeans_plusplus_seeds(X, n_clusters, random_state):
    """scikit-learn's k-means++ seeding (sklearn/cluster/_kmeans.py, ``_kmeans_plusplus`` with its default
    ``n_local_trials = 2 + int(log k)`` and unit sample weights -- what ``KMeans.fit``, and so scripts/learning.py:138, runs
    on the mean-centred rows before its first sweep), restated with NumPy so that the product path does not import
    scikit-learn (0.5 s): the same draws from the same ``RandomState`` (one ``choice``, then ``uniform(size=trials)`` per
    centre), the same expressions in the same order (``-2 X Y^T + |x|^2 + |y|^2`` clipped at 0, ``cumsum`` +
    ``searchsorted``, the greedy choice among the trials).  Pinned to ``sklearn.cluster.kmeans_plusplus`` -- same indices
    -- on the reference matrices and on random ones by tests/test_host_rules.py."""
    X = np.asarray(X, dtype=np.float64)
    n_samples, n_features = X.shape
    x_sq = np.einsum("ij,ij->i", X, X)                       # row_norms(X, squared=True)
    weight = np.ones(n_samples, dtype=np.float64)            # _check_sample_weight(None, X)
    centers = np.empty((n_clusters, n_features), dtype=X.dtype)
    indices = np.full(n_clusters, -1, dtype=int)
    n_local_trials = 2 + int(np.log(n_clusters))

    def sq_dists(A):                                         # _euclidean_distances(A, X, Y_norm_squared=x_sq, squared=True)
        d = -2 * (A @ X.T)
        d += np.einsum("ij,ij->i", A, A)[:, None]
        d += x_sq.reshape(1, -1)
        np.maximum(d, 0, out=d)
        return d

    center_id = random_state.choice(n_samples, p=weight / weight.sum())
    centers[0] = X[center_id]
    indices[0] = center_id
    closest = sq_dists(centers[0, np.newaxis])
    pot = closest @ weight
    for c in range(1, n_clusters):
        rand_vals = random_state.uniform(size=n_local_trials) * pot
        cand = np.searchsorted(np.cumsum(weight * closest, dtype=np.float64), rand_vals)
        np.clip(cand, None, closest.size - 1, out=cand)
        d = sq_dists(X[cand])
        np.minimum(closest, d, out=d)
        cand_pot = d @ weight.reshape(-1, 1)
        best = np.argmin(cand_pot)
        pot = cand_pot[best]
        closest = d[best]
        centers[c] = X[cand[best]]
        indices[c] = cand[best]
    return centers, indices


def _one_blas_thread():
    """The seeding's matrix products are (a few trials) x D by D x n: one thread does them in microseconds, while a BLAS
    pool sized for the whole machine spins on cores the FASTA ingest and the upload are using beside this thread."""
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(1, user_api="blas")
    except ImportError:      # (threadpoolctl comes with scikit-learn; without it the products just run on BLAS's pool)
        import contextlib
        return contextlib.nullcontext()


KMEANS_MIN_GAP = 1e-9   # below this relative distance gap between a point's two nearest centres the host fit decides


def kmeans_reference_on_device(data, k, seed=kmeans_seed, max_iter=300, tol=1e-4, ctx=None):
    """The labels of ``KMeans(n_clusters=k, random_state=seed).fit(data)`` (scripts/learning.py:138) with only the seeding
    on the host: scikit-learn's k-means++ (kmeans_plusplus_seeds, on the mean-centred rows with a fresh
    ``RandomState(seed)`` -- what ``KMeans.fit`` does before its first sweep, n_init = 1) and its Lloyd iteration,
    stopping rule included, on the device (phk_kmeans_lloyd).  Returns (labels, sweeps), or None when a cluster ran
    empty (scikit-learn relocates it) or when some point came within KMEANS_MIN_GAP (relative) of a tie between its two
    nearest centres in some sweep, or when the rows hold a NaN or an infinity: the caller then takes the host fit.

    Parity: the device forms distances by float64 direct differences, scikit-learn by chunked matrix products; the labels
    are EQUAL to scikit-learn 1.7.2's on the reference's matrices (pinned: tests/golden centroids) and on every fold
    subset / random matrix the tests try, and can differ in principle only for points nearer to a tie than the two
    formulations' rounding (~1e-13 relative), which the gap guard hands to the host fit.  Outside those pins: parity
    unpinned (scikit-learn is unpinned by the reference itself, requirements.txt:4)."""
    import ctypes
    X = np.array(data, dtype=np.float64, order="C")          # (a copy: centred in place, as KMeans.fit does)
    n, D = X.shape
    with np.errstate(invalid="ignore"):
        X -= X.mean(axis=0)
        tol_abs = float(np.mean(np.var(X, axis=0)) * tol)
    if not np.isfinite(tol_abs):
        # a NaN or an infinity among the rows (it reaches every entry of its centred column, and so the tolerance, which
        # phk_kmeans_lloyd would refuse as an argument): the host fit refuses such rows with scikit-learn's ValueError
        return None
    with _one_blas_thread():
        init, _ = kmeans_plusplus_seeds(X, int(k), np.random.RandomState(seed))
    init = np.ascontiguousarray(init, dtype=np.float64)
    labels = np.empty(n, dtype=np.uint32)
    n_iter, n_empty, min_gap = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    ctx = ctx or _lib.get_context()
    _lib.check(ctx.lib.phk_kmeans_lloyd(ctx.handle, _lib.ptr(X), n, D, int(k), _lib.ptr(init), tol_abs, int(max_iter), None,
                                        _lib.ptr(labels), ctypes.byref(n_iter), ctypes.byref(n_empty), ctypes.byref(min_gap)))
    if n_empty.value:
        return None
    # a point nearly equidistant from two centres: the device's direct differences and scikit-learn's chunked matrix
    # products (-2 x.c + |c|^2) may order them differently -- such a fit is left to the host
    if not (min_gap.value >= KMEANS_MIN_GAP):
        return None
    return labels.astype(np.int32), n_iter.value


def kmeans(data, k, verbose=False, sort_by_size=False, _ctx=None):
    """K-means labels (scripts/learning.py:131-146), equal to the reference's ``KMeans(n_clusters=k,
    random_state=10).fit(data).labels_``: scikit-learn's seeding on the host, its Lloyd iteration on the device
    (kmeans_reference_on_device).  PHAMERS_KMEANS=sklearn keeps the whole fit on the host, PHAMERS_KMEANS=gpu selects
    the version-independent device k-means (kmeans_gpu: other seeds, other centroids)."""
    import os
    mode = os.environ.get("PHAMERS_KMEANS", "device")
    assignment = None
    if mode == "gpu":
        assignment = kmeans_gpu(data, k)[0]
    elif mode != "sklearn":
        got = kmeans_reference_on_device(data, k, ctx=_ctx)   # (_ctx: a context of the caller's own -- a helper thread's)
        if got is not None:
            assignment = got[0]
    if assignment is None:
        from sklearn.cluster import KMeans
        assignment = KMeans(n_clusters=k, random_state=kmeans_seed).fit(data).labels_
        if type(assignment) != np.ndarray:
            assignment = np.array(assignment)
    if sort_by_size:
        assignment = sort_assignment_by_size(assignment, ascending=False)   # scripts/learning.py:144-145
    return assignment


SEED_MIN_MARGIN = 1e-10   # below this relative margin of a seeding decision the host seeding decides


def placement_draws(n_samples, k, seed=kmeans_seed):
    """The random draws of scikit-learn's k-means++ for ``n_samples`` rows and ``k`` centres from a fresh
    ``RandomState(seed)``: (first centre's row, uniforms (k - 1, 2 + int(ln k))).  They do not depend on the data
    (kmeans_plusplus_seeds: one ``choice`` over uniform weights, then one ``uniform(size=trials)`` per centre)."""
    rs = np.random.RandomState(seed)
    weight = np.ones(n_samples, dtype=np.float64)
    first = int(rs.choice(n_samples, p=weight / weight.sum()))
    trials = 2 + int(np.log(k))
    draws = np.array([rs.uniform(size=trials) for _ in range(1, k)], dtype=np.float64).reshape(k - 1, trials)
    return first, draws


def _place_on_host(reference, contig, k):
    """One contig the reference's way (scripts/analysis.py:771-776) on the single-problem paths."""
    appended = np.vstack((reference, contig[None, :]))
    assignments = np.asarray(kmeans(appended, k))
    return assignments, cluster_silhouettes(appended, assignments, assignments[-1])


def place_contigs(reference, contigs, k_clusters=86, _chunk=0, _details=None):
    """For every row of ``contigs``: k-means (the reference's ``KMeans(n_clusters=k, random_state=10)``) of the ``reference``
    rows with that row appended, and the silhouettes of the row's cluster -- what scripts/analysis.py:771-776 computes per
    contig -- for all contigs in one batched device call (phk_placement_run; the reference rows go up once).  Returns one
    dict per contig: ``labels`` (n + 1,) int32, scikit-learn's; ``cluster`` = the contig's; ``members`` = the reference
    rows in it; ``silhouettes`` = theirs in row order, the contig's last; ``route``: 'device', or 'host' where the device
    declined (a seeding decision within SEED_MIN_MARGIN of a tie, an assignment within KMEANS_MIN_GAP of one, an empty
    cluster, a contig equal to a reference row) and the contig went through ``kmeans`` + ``cluster_silhouettes`` instead:
    the same results, only slower.  PHAMERS_KMEANS=sklearn sends every contig that way; PHAMERS_KMEANS=gpu (other seeds
    than the reference's) is not supported here."""
    import os
    mode = os.environ.get("PHAMERS_KMEANS", "device")
    if mode == "gpu":
        raise NotImplementedError("place_contigs reproduces the reference's seeds; PHAMERS_KMEANS=gpu selects others")
    X = _check_rows(reference)
    Z = _check_rows(np.asarray(contigs, dtype=np.float64).reshape(-1, X.shape[1]) if np.size(contigs) == 0 else contigs)
    if Z.shape[1] != X.shape[1]:
        raise ValueError("all the input array dimensions except for the concatenation axis must match exactly, but along "
                         "dimension 1, the array at index 0 has size %d and the array at index 1 has size %d"
                         % (X.shape[1], Z.shape[1]))
    n, k = X.shape[0], int(k_clusters)
    if k < 1 or k > n + 1:
        raise ValueError("n_samples=%d should be >= n_clusters=%d." % (n + 1, k))
    B = Z.shape[0]
    if B == 0:
        return []
    out = None
    if mode != "sklearn":
        first, draws = placement_draws(n + 1, k)
        ctx = _lib.get_context()
        pl = _lib.Placement(ctx, X)
        try:
            out = pl.run(Z, k, first, draws, chunk=_chunk)
        finally:
            pl.close()
        if _details is not None:
            _details.update(out)
    records = []
    for b in range(B):
        host = out is None or bool(out["status"][b]) or not (out["seed_margin"][b] >= SEED_MIN_MARGIN) \
            or not (out["min_gap"][b] >= KMEANS_MIN_GAP)
        if host:
            labels, sil = _place_on_host(X, Z[b], k)
            labels = np.asarray(labels).astype(np.int32)
        else:
            labels = out["labels"][b].astype(np.int32)
            sil = out["sil"][b, :out["n_members"][b]].copy()
        cluster = int(labels[-1])
        records.append({"labels": labels, "cluster": cluster, "members": np.flatnonzero(labels[:-1] == cluster),
                        "silhouettes": np.asarray(sil), "route": "host" if host else "device"})
    return records


SWEEP_MAX_K = 2981   # from here on 2 + int(ln k) exceeds the ten seeding trials per centre the device kernels are built for


def _kmeans_seeded(data, k, seed):
    """(labels, sweeps) of ``KMeans(n_clusters=k, random_state=seed).fit(data)`` on the single-problem paths: ``kmeans``'s
    routes (host seeding + device Lloyd, else the host fit) for any seed -- ``kmeans`` itself is pinned to kmeans_seed."""
    import os
    if os.environ.get("PHAMERS_KMEANS", "device") != "sklearn":
        got = kmeans_reference_on_device(data, k, seed=seed)
        if got is not None:
            return got
    from sklearn.cluster import KMeans
    fit = KMeans(n_clusters=k, random_state=seed).fit(data)
    return np.asarray(fit.labels_).astype(np.int32), int(fit.n_iter_)


def _silhouettes_of(data, labels):
    return silhouettes(data, labels)   # (kmeans_sweep has an argument of that name)


def kmeans_sweep(data, k_values, seeds=None, silhouettes=True, _chunk=0, _details=None, _pair_budget=-1):
    """One k-means fit per (k, seed) of ``k_values`` x ``seeds`` (k outermost; ``seeds=None``: the reference's kmeans_seed)
    on the same rows, and the silhouettes of every fit -- the work of scripts/cluster.py:38-47 -- as ONE batched device
    call (phk_sweep_run): the rows go up once, seeding included, and all problems share one pass over the pairs.  Returns
    one dict per problem: ``k``, ``seed``, ``labels`` (n,) int32 equal to ``KMeans(n_clusters=k, random_state=seed)
    .fit(data).labels_``, ``n_iter``, ``silhouettes`` (n,) (None without ``silhouettes``), ``silhouette`` = their np.mean,
    ``route``: 'device', or 'host' where the device declined (a seeding decision within SEED_MIN_MARGIN of a tie, an
    assignment within KMEANS_MIN_GAP of one, an empty cluster), for k >= SWEEP_MAX_K and under PHAMERS_KMEANS=sklearn: such
    a problem goes through the single-problem paths (_kmeans_seeded + silhouettes): the same results, only slower.
    PHAMERS_KMEANS=gpu (other seeds than the reference's) is not supported here."""
    import os
    mode = os.environ.get("PHAMERS_KMEANS", "device")
    if mode == "gpu":
        raise NotImplementedError("kmeans_sweep reproduces the reference's seeds; PHAMERS_KMEANS=gpu selects others")
    X = _check_rows(data)
    n = X.shape[0]
    problems = [(int(k), int(seed)) for k in np.asarray(k_values).ravel().tolist()
                for seed in ([kmeans_seed] if seeds is None else list(seeds))]
    for k, _ in problems:
        if k < 1:
            raise ValueError("The 'n_clusters' parameter of KMeans must be an int in the range [1, inf). Got %d instead." % k)
        if k > n:
            raise ValueError("n_samples=%d should be >= n_clusters=%d." % (n, k))
        if silhouettes and not 2 <= k <= n - 1:
            raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % k)
    on_device = [i for i, (k, _) in enumerate(problems) if mode != "sklearn" and k < SWEEP_MAX_K]
    out = None
    if on_device:
        drawn = [placement_draws(n, problems[i][0], problems[i][1]) for i in on_device]
        ctx = _lib.get_context()
        sw = _lib.Sweep(ctx, X)
        try:
            out = sw.run([problems[i][0] for i in on_device], [d[0] for d in drawn], [d[1] for d in drawn],
                         silhouettes=silhouettes, chunk=_chunk, pair_budget=_pair_budget)
        finally:
            sw.close()
        if _details is not None:
            _details.update(out)
            _details["problems"] = [problems[i] for i in on_device]
    where = {i: j for j, i in enumerate(on_device)}
    records = []
    for i, (k, seed) in enumerate(problems):
        j = where.get(i)
        host = j is None or bool(out["status"][j]) or not (out["seed_margin"][j] >= SEED_MIN_MARGIN) \
            or not (out["min_gap"][j] >= KMEANS_MIN_GAP)
        if host:
            labels, n_iter = _kmeans_seeded(X, k, seed)
            sil = _silhouettes_of(X, labels) if silhouettes else None
        else:
            labels, n_iter = out["labels"][j].astype(np.int32), int(out["n_iter"][j])
            sil = out["sil"][j].copy() if silhouettes else None
        records.append({"k": k, "seed": seed, "labels": np.asarray(labels).astype(np.int32), "n_iter": int(n_iter),
                        "silhouettes": sil, "silhouette": None if sil is None else float(np.mean(sil)),
                        "route": "host" if host else "device"})
    return records


def get_centroids(data, assignment):
    """Mean of the member rows per sorted label, -1 excluded (scripts/learning.py:69-81)."""
    data = np.asarray(data)
    labels = sorted(set(assignment) - set([-1]))
    if len(labels) == 0:
        logger.warning("No clusters assigned to data.")
    return np.array([np.mean(data[assignment == c], axis=0) for c in labels])


def log_density(queries, data, bandwidth=0.1):
    """Gaussian kernel density log-likelihood of each row of ``queries`` (N, D) under ``data`` (M, D): what
    KernelDensity(kernel='gaussian', bandwidth=bandwidth).fit(data).score_samples(queries) returns, (N,) float64,
    computed densely in float64 on the device (phk_kde_log_density)."""
    queries = np.asarray(queries, dtype=np.float64)
    if queries.ndim == 1:
        queries = queries[None, :]
    return _lib.kde_log_density(_lib.get_context(), queries, np.asarray(data, dtype=np.float64), bandwidth)


DENSITY_SWEEP_PER_PASS = _lib.KDE_SWEEP_PER_PASS   # bandwidths one device pass carries through one Gram tile


def density_sweep(queries, data, bandwidths, exclude_self=False, _per_pass=None, _batch_rows=0):
    """``log_density(queries, data, h)`` for every h of ``bandwidths`` -- (B, N) float64, row b for ``bandwidths[b]`` (the
    order as given, duplicates kept), each row bit for bit what ``log_density`` returns -- with the rows uploaded once and
    ONE pass over the pairs per DENSITY_SWEEP_PER_PASS bandwidths (phk_kde_sweep): the pair distances do not depend on
    the bandwidth.  With ``exclude_self`` the queries are the data rows themselves (same shape) and query i is scored
    under the data without row i -- left out by index: an equal row elsewhere still counts -- normalised by M - 1 rows:
    the leave-one-out log-density.  ValueError, before any device work, for NaN input, an empty bandwidth list, a
    bandwidth that is not finite and > 0, ``exclude_self`` with differing shapes or a one-row ``data``.  ``_per_pass``
    (at most DENSITY_SWEEP_PER_PASS) and ``_batch_rows`` are for the tests: bandwidths per device pass and queries per
    device batch; no result depends on either."""
    queries = np.asarray(queries, dtype=np.float64)
    if queries.ndim == 1:
        queries = queries[None, :]
    Q, X, h = _lib.check_kde_sweep_arguments(queries, data, bandwidths, exclude_self)
    if _per_pass is not None and not 1 <= int(_per_pass) <= DENSITY_SWEEP_PER_PASS:
        raise ValueError("_per_pass = %d is not in 1..%d" % (int(_per_pass), DENSITY_SWEEP_PER_PASS))
    return _lib.kde_sweep(_lib.get_context(), Q, X, h, exclude_self=exclude_self, per_pass=_per_pass, batch_rows=_batch_rows)


def get_density(point, data, bandwidth=0.1):
    """Density of ``data`` at one point (scripts/learning.py:107-115): the scalar log-likelihood that
    KernelDensity(kernel='gaussian', bandwidth=bandwidth).fit(data).score_samples([point])[0] returns."""
    return float(log_density(np.asarray(point, dtype=np.float64).reshape(1, -1), data, bandwidth)[0])


def _check_rows(data):
    """float64 C-contiguous 2-D rows; the ValueError scikit-learn raises for NaN / infinite input."""
    X = np.ascontiguousarray(data, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("Expected 2D array, got %dD array instead" % X.ndim)
    if np.isnan(X).any():
        raise ValueError("Input contains NaN.")
    if not np.isfinite(X).all():
        raise ValueError("Input contains infinity or a value too large for dtype('float64').")
    return X


def dbscan(data, eps, min_samples, sort_by_size=False):
    """DBSCAN labels (scripts/learning.py:149-163): what ``DBSCAN(eps=eps, min_samples=min_samples).fit(data).labels_``
    returns, -1 = noise, computed on the device (phk_dbscan: neighbours by float64 direct differences, d <= eps).  With
    ``sort_by_size`` the clusters are relabelled largest first, as the reference does."""
    labels = dbscan_fit(data, eps, min_samples)[0]
    num_clusters = len(set(labels.tolist()) - set([-1]))
    pct_unassigned = 100.0 * np.sum(labels == -1) / float(len(labels)) if len(labels) else 0.0
    logger.debug('%d clusters, %.1f%% unassigned' % (num_clusters, pct_unassigned))
    if sort_by_size:
        labels = sort_assignment_by_size(labels, ascending=False)
    return labels


def dbscan_fit(data, eps, min_samples):
    """(labels_, core_sample_indices_) of ``DBSCAN(eps=eps, min_samples=min_samples).fit(data)``."""
    eps, min_samples = _check_dbscan_parameters(eps, min_samples)
    X = _check_rows(data)
    if X.shape[0] == 0:
        raise ValueError("Found array with 0 sample(s) (shape=%s) while a minimum of 1 is required." % (X.shape,))
    labels, core, _ = _lib.dbscan(_lib.get_context(), X, eps, int(min_samples))
    return labels, np.flatnonzero(core)


def _check_dbscan_parameters(eps, min_samples):
    """dbscan_fit's ValueErrors for one eps / one min_samples; returns them as (float, int)."""
    eps = float(eps)
    if not (np.isfinite(eps) and eps > 0.0):
        raise ValueError("The 'eps' parameter of DBSCAN must be a float in the range (0.0, inf). Got %r instead." % (eps,))
    if isinstance(min_samples, (bool, np.bool_)) or not isinstance(min_samples, (int, np.integer)) or min_samples < 1:
        raise ValueError("The 'min_samples' parameter of DBSCAN must be an int in the range [1, inf). Got %r instead."
                         % (min_samples,))
    return eps, int(min_samples)


DBSCAN_SWEEP_MAX_CELLS = 64   # cells of one device pass (one bit each of a row's core mask)


def dbscan_sweep(data, eps_values, min_samples_values, silhouettes=False, _cells_per_pass=DBSCAN_SWEEP_MAX_CELLS,
                 _tiles_per_launch=0, _details=None):
    """DBSCAN for every cell of the grid ``eps_values`` x ``min_samples_values`` on the same rows -- what a loop of
    ``dbscan_fit`` per cell returns -- with the rows uploaded once and ONE pass over the pairs per stage for up to 64 cells
    (phk_dbscan_sweep; more cells run as several passes over the same resident rows).  Returns one dict per cell in the
    order ``for eps in eps_values: for m in min_samples_values`` (the values as given, duplicates kept): ``eps``,
    ``min_samples``, ``labels`` (n,) int64 (-1 = noise) and ``core_sample_indices`` as ``dbscan_fit`` returns them,
    ``n_clusters``, ``n_core``, ``n_border``, ``n_noise``, ``largest`` (the size of the largest cluster, 0 without one) and
    ``route`` ('device').  The ValueErrors are ``dbscan_fit``'s, raised for every value before any device work; empty value
    lists return [].  With ``silhouettes`` a record also has ``silhouette``: ``silhouette_score`` of the rows with a label
    >= 0, NaN unless 2 <= n_clusters <= (number of such rows) - 1.  That is the existing single-problem pass, once per
    cell: the sweep does not fuse it.  ``_cells_per_pass`` / ``_tiles_per_launch`` / ``_details`` are for the tests: cells
    per device pass, pair tiles per launch, and a dict that receives ``passes`` and per pass the ``launches`` of the count,
    union and border stages."""
    eps_list = [e for e in np.asarray(eps_values, dtype=object).ravel().tolist()]
    ms_list = [m for m in np.asarray(min_samples_values, dtype=object).ravel().tolist()]
    eps_list = [_check_dbscan_parameters(e, 1)[0] for e in eps_list]
    ms_list = [_check_dbscan_parameters(1.0, m)[1] for m in ms_list]
    per_pass = int(_cells_per_pass)
    if not 1 <= per_pass <= DBSCAN_SWEEP_MAX_CELLS:
        raise ValueError("_cells_per_pass = %d is not in 1..%d" % (per_pass, DBSCAN_SWEEP_MAX_CELLS))
    X = _check_rows(data)
    if X.shape[0] == 0:
        raise ValueError("Found array with 0 sample(s) (shape=%s) while a minimum of 1 is required." % (X.shape,))
    cells = [(e, m) for e in eps_list for m in ms_list]
    if not cells:
        return []
    n = X.shape[0]
    records, launches = [], []
    rows = _lib.DbscanRows(_lib.get_context(), X)
    try:
        for c0 in range(0, len(cells), per_pass):
            part = cells[c0:c0 + per_pass]
            out = rows.run([e for e, _ in part], [m for _, m in part], _tiles_per_launch)
            launches.append(out["launches"].tolist())
            for c, (e, m) in enumerate(part):
                labels = out["labels"][c].astype(np.int64)
                core = (out["coremask"] >> np.uint64(c)) & np.uint64(1) != 0
                sizes = np.bincount(labels[labels >= 0], minlength=1)
                n_noise = int(np.count_nonzero(labels < 0))
                n_core = int(np.count_nonzero(core))
                records.append({"eps": e, "min_samples": m, "labels": labels, "core_sample_indices": np.flatnonzero(core),
                                "n_clusters": int(out["n_clusters"][c]), "n_core": n_core, "n_border": n - n_core - n_noise,
                                "n_noise": n_noise, "largest": int(sizes.max()), "route": "device"})
    finally:
        rows.close()
    if _details is not None:
        _details["passes"] = len(launches)
        _details["launches"] = launches
    if silhouettes:
        for record in records:
            clustered = record["labels"] >= 0
            m = int(np.count_nonzero(clustered))
            record["silhouette"] = silhouette_score(X[clustered], record["labels"][clustered]) \
                if 2 <= record["n_clusters"] <= m - 1 else float("nan")
    return records


def kdistances(data, k):
    """The distance from every row of ``data`` to its k-th nearest row, the row itself counting as the first, sorted
    ascending: the usual curve for choosing DBSCAN's eps by eye.  From ``kneighbors(data, data, k)``, so 1 <= k <= 28 and the
    distances are the direct-difference ones ``dbscan`` and ``dbscan_sweep`` decide on: a row is a core sample at
    (eps, min_samples) exactly when its min_samples-th distance is <= eps."""
    data = np.asarray(data, dtype=np.float64)
    d, _ = kneighbors(data, data, k)
    return np.sort(d[:, int(k) - 1])


def silhouettes(data, assignment):
    """Silhouette value of every row (scripts/learning.py:84-92): what ``silhouette_samples(data, assignment)`` returns.
    Labels of any type are encoded in np.unique order (scikit-learn's LabelEncoder); -1 is an ordinary cluster here.
    Computed on the device (phk_silhouettes), float64, bit-identical from run to run."""
    X = _check_rows(data)
    assignment = np.asarray(assignment)
    if assignment.shape != (X.shape[0],):
        raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]"
                         % (X.shape[0], assignment.shape[0] if assignment.ndim else 1))
    _, codes = np.unique(assignment, return_inverse=True)
    codes = codes.ravel()
    n_labels = int(codes.max()) + 1 if codes.size else 0
    if not 2 <= n_labels <= X.shape[0] - 1:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % n_labels)
    return _lib.silhouettes(_lib.get_context(), X, codes, n_labels)


def cluster_silhouettes(data, assignment, cluster):
    """Silhouettes of the members of one cluster, in row order (scripts/learning.py:95-104)."""
    ss = silhouettes(data, assignment)
    return np.array([ss[i] for i in range(len(assignment)) if assignment[i] == cluster])


def silhouette_score(data, labels):
    """Mean silhouette (sklearn.metrics.silhouette_score with its defaults, as scripts/cluster.py:43 calls it)."""
    return float(np.mean(silhouettes(data, labels)))


def cluster_deviations(data, assignment):
    """Mean distance of each cluster's members to its centroid (scripts/learning.py:31-44), replicated as written: the
    clusters are taken to be labelled 0..K-1 (K = the number of labels other than -1)."""
    data = np.asarray(data)
    num_clusters = len(set(assignment) - set([-1]))
    centroids = get_centroids(data, assignment)
    deviations = np.zeros(num_clusters)
    for cluster in range(num_clusters):
        which = [i for i in range(data.shape[0]) if assignment[i] == cluster]
        vector = centroids[cluster]
        if len(vector.shape) == 1:
            vector = np.array([vector])
        deviations[cluster] = np.mean(np.linalg.norm(np.repeat(vector, data[which].shape[0], axis=0) - data[which], axis=1))
    return deviations


def sort_assignment_by_size(assignment, ascending=True):
    """Clusters relabelled by size (scripts/learning.py:166-182): 0 = the smallest when ``ascending``, the largest
    otherwise; ties in the order of ``sorted(zip(sizes, clusters))`` (reversed when not ascending); -1 stays -1."""
    assignment = np.asarray(assignment)
    cluster_set = list(set(assignment.tolist()) - set([-1]))
    cluster_sizes = [np.sum(assignment == cluster) for cluster in cluster_set]
    sorted_assignment = [cluster for (size, cluster) in sorted(zip(cluster_sizes, cluster_set))[::[-1, 1][ascending]]]
    new_assignment = np.ones(len(assignment), dtype=int) * -1
    for new, cluster in enumerate(sorted_assignment):
        new_assignment[assignment == cluster] = new
    return new_assignment


# ---- evaluation of score vectors (scripts/learning.py:185-243) -----------------------------------------------------------
METRIC_NAMES = ('tp', 'fp', 'fn', 'tn', 'tpr', 'fpr', 'fnr', 'tnr', 'ppv', 'npv', 'fdr', 'acc')   # scripts/learning.py:232


class Metrics(dict):
    """The reference's twelve prediction metrics in its order, by key or by attribute (``m['tpr']``, ``m.tpr``): what
    scripts/learning.py:223-243 returns as a pandas Series, without pandas."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = value


def _scores_1d(scores):
    return np.ascontiguousarray(np.asarray(scores, dtype=np.float64).ravel())


def _scores_and_labels(positive_scores, negative_scores):
    pos, neg = _scores_1d(positive_scores), _scores_1d(negative_scores)
    labels = np.zeros(len(pos) + len(neg), dtype=np.uint8)
    labels[:len(pos)] = 1
    return np.concatenate((pos, neg)), labels


def argsort_scores(scores, descending=False):
    """The stable permutation that orders ``scores``: ``np.argsort(scores, kind='stable')``, or of ``-scores`` when
    ``descending`` (ties stay in index order both ways), sorted on the device (phk_argsort_f64).  ValueError for NaN or
    infinite scores."""
    x = _scores_1d(scores)
    perm = np.empty(len(x), dtype=np.uint32)
    ctx = _lib.get_context()
    rc = ctx.lib.phk_argsort_f64(ctx.handle, _lib.ptr(x), len(x), 1 if descending else 0, _lib.ptr(perm))
    if rc == _lib.PHK_ERR_NAN:
        raise ValueError("Input contains NaN or infinity.")
    _lib.check(rc)
    return perm.astype(np.int64)


def roc_points(scores, labels, drop_intermediate=True, _device=None):
    """scikit-learn's ``roc_curve(labels, scores, drop_intermediate=...)`` before its divisions (phk_roc_curve): (fps, tps,
    thresholds, area2) with integer fps / tps (uint64) and area2 = 2 P N AUC as a Python int.  ``_device`` = (d_scores,
    d_labels, n): device pointers of resident scores (float64) and labels (uint8) instead (phk_roc_curve_dev)."""
    import ctypes
    ctx = _lib.get_context()
    if _device is None:
        x = _scores_1d(scores)
        lab = np.ascontiguousarray(np.asarray(labels).ravel() != 0, dtype=np.uint8)
        if lab.shape != x.shape:
            raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]" % (len(lab), len(x)))
        n, fn, a, b = len(x), ctx.lib.phk_roc_curve, _lib.ptr(x), _lib.ptr(lab)
    else:
        a, b, n = _device
        fn, a, b = ctx.lib.phk_roc_curve_dev, ctypes.c_void_p(int(a)), ctypes.c_void_p(int(b))
    fps, tps = np.empty(n + 1, dtype=np.uint64), np.empty(n + 1, dtype=np.uint64)
    thresholds = np.empty(n + 1, dtype=np.float64)
    m, area2 = ctypes.c_uint64(), ctypes.c_uint64()
    rc = fn(ctx.handle, a, b, n, 1 if drop_intermediate else 0, _lib.ptr(fps), _lib.ptr(tps), _lib.ptr(thresholds),
            ctypes.byref(m), ctypes.byref(area2))
    if rc == _lib.PHK_ERR_NAN:
        raise ValueError("Input contains NaN or infinity.")   # scikit-learn's roc_curve raises on such scores too
    _lib.check(rc)
    return fps[:m.value].copy(), tps[:m.value].copy(), thresholds[:m.value].copy(), int(area2.value)


def rates_from_points(fps, tps, area2):
    """(fpr, tpr, auc) from the integer curve: scikit-learn's own divisions ``fps / fps[-1]``, ``tps / tps[-1]`` (bit-identical
    rates), and auc = area2 / (2 P N), one rounding of the exact area.  A class without members gives NaN rates and a NaN
    area, as scikit-learn does (with its warning)."""
    fps, tps = np.asarray(fps, dtype=np.float64), np.asarray(tps, dtype=np.float64)
    n_neg, n_pos = int(fps[-1]), int(tps[-1])
    fpr = fps / fps[-1] if n_neg else np.full(fps.shape, np.nan)
    tpr = tps / tps[-1] if n_pos else np.full(tps.shape, np.nan)
    auc = int(area2) / (2 * n_pos * n_neg) if n_pos and n_neg else float('nan')   # (Python's int / int rounds once)
    return fpr, tpr, auc


def predictor_performance(positive_scores, negative_scores):
    """(false positive rate, true positive rate, ROC area) of a scoring (scripts/learning.py:185-196): scikit-learn's
    ``roc_curve`` -- the rates bit-identical to it -- and ``auc``, from a sort and integer scans on the device."""
    scores, labels = _scores_and_labels(positive_scores, negative_scores)
    fps, tps, _, area2 = roc_points(scores, labels)
    return rates_from_points(fps, tps, area2)


def truth_counts(positive_scores, negative_scores, threshold=0):
    """(tp, fp, fn, tn) at ``threshold``, >= / < as scripts/learning.py:206-209, counted on the device (phk_truth_counts)."""
    scores, labels = _scores_and_labels(positive_scores, negative_scores)
    counts = np.zeros(4, dtype=np.uint64)
    ctx = _lib.get_context()
    rc = ctx.lib.phk_truth_counts(ctx.handle, _lib.ptr(scores), _lib.ptr(labels), len(scores), float(threshold), _lib.ptr(counts))
    if rc == _lib.PHK_ERR_ARG:
        raise ValueError(_lib.last_error())
    _lib.check(rc)
    return tuple(int(c) for c in counts)


def _rates(tp, fp, fn, tn):
    tpr = float(tp) / (tp + fn) if tp + fn != 0 else 0      # scripts/learning.py:210-217
    fpr = float(fp) / (fp + tn) if fp + tn != 0 else 0
    return tpr, fpr, 1 - tpr, 1 - fpr


def get_truth_table(positive_scores, negative_scores, threshold=0):
    """(TPR, FPR, FNR, TNR) at ``threshold`` (scripts/learning.py:199-220)."""
    return _rates(*truth_counts(positive_scores, negative_scores, threshold))


def get_predictor_metrics(positive_scores, negative_scores, threshold=0):
    """The reference's metrics (scripts/learning.py:223-243) as a ``Metrics`` mapping in its order: tp, fp, fn, tn, tpr, fpr,
    fnr, tnr, ppv, npv, fdr, acc.  The counts are floats, as the cells of the reference's Series are.  ZeroDivisionError
    where the reference raises it (nothing scored at or above / below the threshold)."""
    tp, fp, fn, tn = truth_counts(positive_scores, negative_scores, threshold)
    m = Metrics()
    m.tp, m.fp, m.fn, m.tn = float(tp), float(fp), float(fn), float(tn)
    m.tpr, m.fpr, m.fnr, m.tnr = _rates(tp, fp, fn, tn)
    m.ppv = float(m.tp) / (m.tp + m.fp)
    m.npv = float(m.tn) / (m.tn + m.fn)
    m.fdr = 1 - m.ppv
    m.acc = float(m.tp + m.tn) / (m.tp + m.fp + m.fn + m.tn)
    return m
