"""GPU: DBSCAN and silhouettes (cluster.hip) against the reference's scikit-learn results (tests/golden/clustering.npz,
tools/gen_golden_cluster.py) and against the NumPy restatement (tests/cluster_ref.py).  Bars: DBSCAN labels and core points
identical; silhouettes within 1e-8 of scikit-learn and of the restatement, bit-identical from run to run."""
import numpy as np
import pytest

from tests import cluster_ref, helpers

pytestmark = pytest.mark.gpu
SKL = 1e-8


def _classes():
    from oracle import oracle
    ref = helpers.load_npz("ref_features.npz")
    return {"pos": oracle.normalize_counts(ref["pos_counts"].astype(np.int64)),
            "neg": oracle.normalize_counts(ref["neg_counts"].astype(np.int64))}


def _check_dbscan(g, tag, X, eps, ms):
    from phamers_amd import learning
    labels, core = learning.dbscan_fit(X, eps, ms)
    assert np.array_equal(labels, g[tag + "_labels"]), tag
    assert np.array_equal(core, g[tag + "_core"]), tag
    assert np.array_equal(learning.dbscan(X, eps, ms), g[tag + "_labels"]), tag


@pytest.mark.parametrize("cls", ["pos", "neg"])
def test_dbscan_equals_scikit_learn_on_the_reference_rows(cls):
    g = helpers.load_npz("clustering.npz")
    X = _classes()[cls]
    for i, (eps, ms) in enumerate(g["dbscan_cases"]):
        _check_dbscan(g, "dbscan_%s_%d" % (cls, i), X, float(eps), int(ms))


def test_dbscan_equals_scikit_learn_on_the_synthetic_sets():
    g = helpers.load_npz("clustering.npz")
    B = g["blobs"]
    _check_dbscan(g, "dbscan_blobs", B, 0.6, 5)
    _check_dbscan(g, "dbscan_blobs_ms1", B, 0.3, 1)
    _check_dbscan(g, "dbscan_blobs_noise", B, 0.6, B.shape[0] + 1)
    for order in ("apb", "bpa", "pba"):
        _check_dbscan(g, "dbscan_tie_" + order, cluster_ref.border_tie(order), 0.9, 4)
    _check_dbscan(g, "dbscan_dyadic", g["dyadic"], 5.0, 2)      # |(3,4) - (0,0)| = 5 = eps: neighbours


def test_dbscan_sort_by_size_matches_the_reference():
    from phamers_amd import learning
    g = helpers.load_npz("clustering.npz")
    for c, X in _classes().items():
        for i in (0, 3):
            eps, ms = g["dbscan_cases"][i]
            got = learning.dbscan(X, float(eps), int(ms), sort_by_size=True)
            assert np.array_equal(got, g["sorted_dbscan_%s_%d" % (c, i)])


def test_silhouettes_match_scikit_learn_and_repeat_bit_for_bit():
    from phamers_amd import learning
    g = helpers.load_npz("clustering.npz")
    case = int(g["sil_dbscan_case"][0])
    for c, X in _classes().items():
        km = g["kmeans_%s" % c]
        s1 = learning.silhouettes(X, km)
        assert np.abs(s1 - g["sil_kmeans_%s" % c]).max() <= SKL
        assert np.array_equal(s1, learning.silhouettes(X, km))
        assert abs(learning.silhouette_score(X, km) - g["score_kmeans_%s" % c][0]) <= SKL
        assert np.abs(learning.cluster_silhouettes(X, km, 0) - g["csil_kmeans_%s" % c]).max() <= SKL
        dl = g["dbscan_%s_%d_labels" % (c, case)]
        assert np.abs(learning.silhouettes(X, dl) - g["sil_dbscan_%s" % c]).max() <= SKL
        assert np.abs(learning.cluster_silhouettes(X, dl, -1) - g["csil_dbscan_%s_noise" % c]).max() <= SKL
        assert np.abs(learning.cluster_deviations(X, km) - g["dev_kmeans_%s" % c]).max() <= 1e-12
    B = g["blobs"]
    assert np.abs(learning.silhouettes(B, g["blobs_sparse_labels"]) - g["sil_blobs_sparse"]).max() <= SKL
    assert np.abs(learning.cluster_silhouettes(B, g["blobs_sparse_labels"], 7) - g["csil_blobs_sparse_7"]).max() <= SKL
    single = learning.silhouettes(B, g["blobs_single_labels"])
    assert np.abs(single - g["sil_blobs_single"]).max() <= SKL and np.all(single[[5, 17, 40]] == 0.0)


@pytest.mark.parametrize("n, D, K", [(700, 2, 5), (333, 1024, 4), (150, 4096, 3), (1000, 37, 300)])
def test_silhouettes_match_the_restatement_on_random_data(n, D, K):
    from phamers_amd import learning
    rng = np.random.default_rng(n + D)
    X = rng.random((n, D))
    lab = rng.integers(0, K, n) * 3 - 1            # non-contiguous labels, -1 included
    got = learning.silhouettes(X, lab)
    assert np.abs(got - cluster_ref.silhouettes(X, lab)).max() <= SKL
    assert np.array_equal(got, learning.silhouettes(X, lab))


@pytest.mark.parametrize("D", [2, 1024, 4096])
def test_dbscan_matches_the_restatement_at_every_width(D):
    from phamers_amd import learning
    rng = np.random.default_rng(D)
    n = 400 if D > 2 else 1500
    centres = rng.random((5, D)) * 4.0
    X = centres[rng.integers(0, 5, n)] + rng.normal(size=(n, D)) * (0.3 / np.sqrt(D))
    eps = 0.25
    assert cluster_ref.eps_margin(X, eps) > 1e-9
    want, core = cluster_ref.dbscan(X, eps, 4)
    labels, got_core = learning.dbscan_fit(X, eps, 4)
    assert np.array_equal(labels, want) and np.array_equal(got_core, np.flatnonzero(core))


def test_kmeans_sort_by_size_matches_the_reference():
    from phamers_amd import learning
    g = helpers.load_npz("clustering.npz")
    X = _classes()["pos"]
    got = learning.kmeans(X, int(g["k_clusters"][0]), sort_by_size=True)
    assert np.array_equal(got, g["sorted_kmeans_pos_desc"])


# ---- scale: beyond what scikit-learn can run ----------------------------------------------------------------------------

def test_dbscan_scale_2_17_rows_in_64_blobs():
    from phamers_amd import learning
    rng = np.random.default_rng(17)
    n, D, k = 1 << 17, 8, 64
    centres = np.zeros((k, D))
    centres[:, 0] = np.arange(k) * 10.0                           # 10 apart; blob radius < 0.5
    member = rng.integers(0, k, n)
    X = centres[member] + rng.uniform(-0.1, 0.1, (n, D))
    labels = learning.dbscan(X, 1.0, 5)
    _, first = np.unique(member, return_index=True)
    rank = np.empty(k, dtype=np.int64)
    rank[np.argsort(first)] = np.arange(k)                        # clusters numbered by first occurrence
    assert np.array_equal(labels, rank[member])


def test_dbscan_scale_eps_one_on_normalised_rows():
    from phamers_amd import _lib
    rng = np.random.default_rng(1)
    n = 1 << 17
    X = rng.random((n, 64))
    X /= X.sum(axis=1, keepdims=True)                               # pairwise distances < sqrt(2) x max row norm << 1
    labels, core, k = _lib.dbscan(_lib.get_context(), X, 1.0, 2)
    assert k == 1 and core.all() and np.all(labels == 0)


def test_dbscan_chain_of_2_16_points():
    """A chain spaced 0.9 eps: union-find must join 2^16 links; the two ends have 2 neighbours < 3 and are border points."""
    from phamers_amd import learning
    n = 1 << 16
    X = np.zeros((n, 2))
    X[:, 0] = np.arange(n) * 0.9
    perm = np.random.default_rng(2).permutation(n)
    labels, core = learning.dbscan_fit(X[perm], 1.0, 3)
    assert np.all(labels == 0)
    mask = np.zeros(n, dtype=bool)
    mask[core] = True
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    assert not mask[inv[0]] and not mask[inv[n - 1]] and mask.sum() == n - 2


def test_silhouettes_scale_2_16_rows_sampled():
    from phamers_amd import learning
    rng = np.random.default_rng(16)
    n, D, K = 1 << 16, 16, 50
    X = rng.random((n, D))
    lab = rng.integers(0, K, n)
    X += lab[:, None] * 0.05
    got = learning.silhouettes(X, lab)
    rows = rng.choice(n, 512, replace=False)
    assert np.abs(got[rows] - cluster_ref.silhouettes_sample(X, lab, rows)).max() <= SKL


# ---- several launches and odd shapes --------------------------------------------------------------------------------------

def _profiled(ctx, fn):
    """fn() with the profiler on: (its result, {kernel: launches})."""
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        out = fn()
        return out, {k: v[1] for k, v in ctx.profile().items()}
    finally:
        ctx.profile_enable(False)


def _chains(n_pairs=24, length=3500):
    """Dyadic 2-D rows for eps = 1, min_samples = 4 (every distance exact, d = eps included): pairs of parallel chains
    spaced 0.5 (chain A at y = 4k, chain B at y = 4k + 2); every other pair joined at its far end by three rows; border
    rows at y = 4k + 1, exactly eps from one core row of each chain of an unjoined pair (three neighbours: not core); noise
    rows 3 apart below everything."""
    x = np.arange(length) * 0.5
    rows = []
    for k in range(n_pairs):
        y0 = 4.0 * k
        for yy in (y0, y0 + 2.0):
            rows.append(np.column_stack((x, np.full(length, yy))))
        if k % 2:
            rows.append(np.column_stack((np.full(3, x[-1]), y0 + np.array([0.5, 1.0, 1.5]))))
        else:
            bx = x[np.arange(3, length - 3, 701)]
            rows.append(np.column_stack((bx, np.full(len(bx), y0 + 1.0))))
    rows.append(np.column_stack((np.arange(1000) * 3.0, np.full(1000, -10.0))))
    return np.vstack(rows)


def test_dbscan_union_in_several_launches():
    """More than 2^17 + 2^15 core rows: the union pass runs in at least two launches (the row blocks I of a later launch
    start at ib0 > 0).  Components spread over every slice (permuted rows), chains joined at one far end, border rows between
    two clusters (the smaller label wins) and noise: labels and core mask equal the cell-list restatement."""
    from phamers_amd import _lib
    X = _chains()
    X = X[np.random.default_rng(7).permutation(len(X))]
    want, want_core = cluster_ref.dbscan_cells(X, 1.0, 4)
    assert want_core.sum() >= (1 << 17) + (1 << 15)
    assert (want == -1).sum() == 1000 and want.max() + 1 == 36
    ctx = _lib.get_context()
    (labels, core, k), launches = _profiled(ctx, lambda: _lib.dbscan(ctx, X, 1.0, 4))
    assert launches["phk_cl_union_kernel"] >= 2, launches
    assert k == want.max() + 1
    assert np.array_equal(core, want_core)
    assert np.array_equal(labels, want)


def test_dbscan_cell_restatement_sees_two_labelled_borders():
    """(the scale case above is only as good as its borders: some border rows do touch two clusters)"""
    X = _chains(n_pairs=2, length=40)
    labels, core = cluster_ref.dbscan_cells(X, 1.0, 4)
    d = cluster_ref.pair_distances(X, X)
    border = np.flatnonzero(~core & (labels >= 0))
    two = [i for i in border if len(set(labels[(d[i] <= 1.0) & core].tolist())) == 2]
    assert two and all(labels[i] == min(labels[(d[i] <= 1.0) & core]) for i in two)


@pytest.mark.parametrize("D", [1, 15, 16, 17])
def test_dbscan_small_shapes(D):
    """n around the 64-row tile, D around the 16-column LDS step, min_samples in {1, 2, 5, n, n + 1}, exact duplicates:
    labels and core rows equal cluster_ref.dbscan."""
    from phamers_amd import learning
    rng = np.random.default_rng(100 + D)
    eps = 0.25 * np.sqrt(D) + 0.125
    for n in (1, 2, 63, 64, 65, 129):
        X = rng.integers(0, 4, (n, D)) / 4.0
        X[n // 2:n // 2 + n // 4] = X[:n // 4]
        for ms in sorted({1, 2, 5, n, n + 1}):
            want, want_core = cluster_ref.dbscan(X, eps, ms)
            labels, core = learning.dbscan_fit(X, eps, ms)
            assert np.array_equal(labels, want), (n, ms)
            assert np.array_equal(core, np.flatnonzero(want_core)), (n, ms)


def test_silhouettes_in_several_query_batches():
    """K = 4 096 labels cap a query batch at 8 192 rows: 40 000 rows run in five batches, the last one partial (the finish
    kernel's and the sums kernel's q0 > 0).  Singletons score 0; clusters larger than 64 rows span several chunks.  Sampled
    rows (B - 1, B, B + 1 and the last row among them) within 1e-8 of the restatement; a second call is bit-identical."""
    from phamers_amd import _lib, learning
    rng = np.random.default_rng(40)
    n, K = 40000, 4096
    lab = np.concatenate((np.repeat(np.arange(20), 300), np.arange(20, 120), 120 + np.arange(n - 6100) % (K - 120)))
    lab = lab[rng.permutation(n)]
    assert len(np.unique(lab)) == K
    X = rng.random((n, 2)) + (lab % 16)[:, None] * 0.25
    ctx = _lib.get_context()
    got, launches = _profiled(ctx, lambda: learning.silhouettes(X, lab))
    assert launches["phk_cl_silhouette_finish_kernel"] >= 2, launches
    single = np.flatnonzero(np.bincount(lab, minlength=K)[lab] == 1)
    assert len(single) >= 100 and np.all(got[single] == 0.0)
    B = 8192
    rows = np.unique(np.concatenate(([0, B - 1, B, B + 1, 2 * B, n - 1], rng.choice(n, 200, replace=False))))
    assert np.abs(got[rows] - cluster_ref.silhouettes_sample(X, lab, rows)).max() <= SKL
    assert np.array_equal(learning.silhouettes(X, lab), got)


@pytest.mark.parametrize("D", [1, 16, 17])
def test_silhouettes_with_unused_label_ids(D):
    """phk_silhouettes with label ids that have no members (sizes[c] = 0): empty clusters take no part in b; the result
    equals that of the same clusters numbered without gaps."""
    from phamers_amd import _lib
    rng = np.random.default_rng(D)
    n = 300
    X = rng.random((n, D))
    used = np.array([1, 4, 5, 9])
    lab = used[rng.integers(0, 4, n)]
    X += (lab == 4)[:, None] * 0.5
    ctx = _lib.get_context()
    got = _lib.silhouettes(ctx, X, lab, 12)
    dense = np.searchsorted(used, lab)
    assert np.array_equal(got, _lib.silhouettes(ctx, X, dense, 4))
    assert np.abs(got - cluster_ref.silhouettes(X, lab)).max() <= SKL
