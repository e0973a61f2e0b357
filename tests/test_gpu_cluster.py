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
