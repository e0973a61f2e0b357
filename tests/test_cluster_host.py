"""CPU: the clustering fixture (tests/golden/clustering.npz, tools/gen_golden_cluster.py) against the NumPy restatement
(tests/cluster_ref.py), the C ABI declarations, and the argument checks of learning.dbscan / silhouettes, without a device."""
import numpy as np
import pytest

from tests import cluster_ref, helpers

SKL = 1e-8


def _classes():
    from oracle import oracle
    ref = helpers.load_npz("ref_features.npz")
    return {"pos": oracle.normalize_counts(ref["pos_counts"].astype(np.int64)),
            "neg": oracle.normalize_counts(ref["neg_counts"].astype(np.int64))}


def _core_mask(g, tag, n):
    m = np.zeros(n, dtype=bool)
    m[g[tag + "_core"]] = True
    return m


def test_restated_dbscan_equals_the_fixture_on_the_reference_rows():
    g = helpers.load_npz("clustering.npz")
    assert str(g["sklearn_version"])
    for c, X in _classes().items():
        for i, (eps, ms) in enumerate(g["dbscan_cases"]):
            tag = "dbscan_%s_%d" % (c, i)
            assert g[tag + "_margin"][0] >= 1e-9
            labels, core = cluster_ref.dbscan(X, float(eps), int(ms))
            assert np.array_equal(labels, g[tag + "_labels"]), tag
            assert np.array_equal(core, _core_mask(g, tag, X.shape[0])), tag


def test_restated_dbscan_equals_the_fixture_on_the_synthetic_sets():
    g = helpers.load_npz("clustering.npz")
    cases = {"blobs": (g["blobs"], 0.6, 5), "blobs_ms1": (g["blobs"], 0.3, 1),
             "blobs_noise": (g["blobs"], 0.6, g["blobs"].shape[0] + 1), "dyadic": (g["dyadic"], 5.0, 2)}
    for order in ("apb", "bpa", "pba"):
        cases["tie_" + order] = (cluster_ref.border_tie(order), 0.9, 4)
    for name, (X, eps, ms) in cases.items():
        tag = "dbscan_" + name
        labels, core = cluster_ref.dbscan(X, eps, ms)
        assert np.array_equal(labels, g[tag + "_labels"]), tag
        assert np.array_equal(core, _core_mask(g, tag, X.shape[0])), tag
    assert np.all(g["dbscan_blobs_noise_labels"] == -1) and g["dbscan_blobs_noise_core"].size == 0
    assert g["dbscan_blobs_ms1_core"].size == g["blobs"].shape[0]
    assert np.array_equal(g["dbscan_dyadic_labels"], [0, 0, 0])      # d = eps exactly is a neighbour
    # the border point takes the smaller label of its two clusters, whichever comes first in row order
    assert g["dbscan_tie_apb_labels"][4] == 0 and g["dbscan_tie_bpa_labels"][4] == 0 and g["dbscan_tie_pba_labels"][0] == 0


def test_restated_silhouettes_equal_the_fixture():
    g = helpers.load_npz("clustering.npz")
    for c, X in _classes().items():
        sk = cluster_ref.silhouettes(X, g["kmeans_%s" % c])
        assert np.abs(sk - g["sil_kmeans_%s" % c]).max() <= SKL
        dl = g["dbscan_%s_%d_labels" % (c, int(g["sil_dbscan_case"][0]))]
        assert np.abs(cluster_ref.silhouettes(X, dl) - g["sil_dbscan_%s" % c]).max() <= SKL
    X = g["blobs"]
    assert np.abs(cluster_ref.silhouettes(X, g["blobs_sparse_labels"]) - g["sil_blobs_sparse"]).max() <= SKL
    single = cluster_ref.silhouettes(X, g["blobs_single_labels"])
    assert np.abs(single - g["sil_blobs_single"]).max() <= SKL
    assert np.all(single[[5, 17, 40]] == 0.0)


def test_sort_assignment_by_size_equals_the_fixture():
    from phamers_amd import learning
    g = helpers.load_npz("clustering.npz")
    for c in ("pos", "neg"):
        km = g["kmeans_%s" % c]
        assert np.array_equal(learning.sort_assignment_by_size(km), g["sorted_kmeans_%s_asc" % c])
        assert np.array_equal(learning.sort_assignment_by_size(km, ascending=False), g["sorted_kmeans_%s_desc" % c])
        assert np.array_equal(cluster_ref.sort_assignment_by_size(km), g["sorted_kmeans_%s_asc" % c])
        for i in range(len(g["dbscan_cases"])):
            lab = g["dbscan_%s_%d_labels" % (c, i)]
            assert np.array_equal(learning.sort_assignment_by_size(lab, ascending=False), g["sorted_dbscan_%s_%d" % (c, i)])


def test_cluster_deviations_equals_the_fixture():
    """cluster_deviations is NumPy on the host: no device needed."""
    from phamers_amd import learning
    g = helpers.load_npz("clustering.npz")
    for c, X in _classes().items():
        assert np.abs(learning.cluster_deviations(X, g["kmeans_%s" % c]) - g["dev_kmeans_%s" % c]).max() <= 1e-12
        dl = g["dbscan_%s_%d_labels" % (c, int(g["sil_dbscan_case"][0]))]
        assert np.abs(learning.cluster_deviations(X, dl) - g["dev_dbscan_%s" % c]).max() <= 1e-12


def test_binding_and_header_declare_the_cluster_entries():
    from phamers_amd import _lib
    c_int, c_double = _lib.c_int, _lib.c_double
    res, args = _lib.SIGNATURES["phk_silhouettes"]
    assert res is c_int and len(args) == 7 and args[5] is _lib.c_u32
    res, args = _lib.SIGNATURES["phk_dbscan"]
    assert res is c_int and len(args) == 9 and args[4] is c_double
    text = open(helpers.os.path.join(helpers.REPO, "include", "phamers_hip.h")).read()
    assert "int phk_silhouettes(phk_ctx *ctx," in text and "int phk_dbscan(phk_ctx *ctx," in text
    assert "#define PHK_ABI_VERSION 2" in text


@pytest.fixture
def no_device(monkeypatch):
    from phamers_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("device work for bad input")
    monkeypatch.setattr(_lib, "get_context", refuse)


@pytest.mark.parametrize("eps, ms", [(0.0, 2), (-1.0, 2), (float("nan"), 2), (float("inf"), 2), (0.5, 0), (0.5, -3), (0.5, 2.5)])
def test_dbscan_bad_arguments_raise_before_device_work(no_device, eps, ms):
    from phamers_amd import learning
    with pytest.raises(ValueError):
        learning.dbscan(np.zeros((4, 2)), eps, ms)


def test_nan_input_raises_before_device_work(no_device):
    from phamers_amd import learning
    X = np.arange(20, dtype=np.float64).reshape(10, 2)
    X[3, 1] = np.nan
    lab = np.arange(10) % 3
    for call in (lambda: learning.dbscan(X, 0.5, 2), lambda: learning.silhouettes(X, lab),
                 lambda: learning.silhouette_score(X, lab), lambda: learning.cluster_silhouettes(X, lab, 1)):
        with pytest.raises(ValueError, match="Input contains NaN."):
            call()


@pytest.mark.parametrize("labels", [np.zeros(6, dtype=int), np.arange(6)])
def test_silhouettes_label_count_is_checked_before_device_work(no_device, labels):
    from phamers_amd import learning
    with pytest.raises(ValueError, match="Number of labels is %d" % len(set(labels))):
        learning.silhouettes(np.random.RandomState(0).rand(6, 3), labels)
    with pytest.raises(ValueError, match="Number of labels"):
        cluster_ref.silhouettes(np.random.RandomState(0).rand(6, 3), labels)


def test_kmeans_sort_by_size_relabels_largest_first(monkeypatch):
    """kmeans(sort_by_size=True) no longer raises: it relabels as scripts/learning.py:144-145 does (fit stubbed here)."""
    from phamers_amd import learning
    fit = np.array([2, 0, 0, 1, 1, 1, 2, 1])
    monkeypatch.setenv("PHAMERS_KMEANS", "gpu")
    monkeypatch.setattr(learning, "kmeans_gpu", lambda data, k: (fit.copy(), None, 1))
    got = learning.kmeans(np.zeros((8, 2)), 3, sort_by_size=True)
    assert np.array_equal(got, cluster_ref.sort_assignment_by_size(fit, ascending=False))
    assert np.array_equal(got, [1, 2, 2, 0, 0, 0, 1, 0])


@pytest.mark.parametrize("D", [1, 2, 3])
def test_cell_list_dbscan_equals_the_all_pairs_restatement(D):
    """cluster_ref.dbscan_cells (the scalable restatement the GPU scale test is held to) against cluster_ref.dbscan on random
    and dyadic sets with exact duplicates, eps on and off the dyadic grid."""
    rng = np.random.default_rng(D)
    for trial in range(8):
        n = int(rng.integers(1, 400))
        X = rng.integers(0, 16, (n, D)) / 8.0 if trial % 2 else rng.random((n, D)) * 2.0 - 0.5
        X[n // 2:n // 2 + n // 4] = X[:n // 4]
        for eps in (0.125, 0.25, 0.3, 0.5, 1.0):
            for ms in (1, 2, 4, 7):
                a, ca = cluster_ref.dbscan(X, eps, ms)
                b, cb = cluster_ref.dbscan_cells(X, eps, ms)
                assert np.array_equal(a, b) and np.array_equal(ca, cb), (trial, eps, ms)
