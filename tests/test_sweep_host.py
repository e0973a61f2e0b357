"""The k-means sweep's host side, no GPU: the problem order and the argument errors of learning.kmeans_sweep (raised before
any device work), silhouette_curve's arithmetic on canned records, the curve file, and the NumPy restatement
tests/sweep_ref.py against scikit-learn."""
import numpy as np
import pytest

from tests import sweep_ref


def _blobs(n, D, seed):
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-1, 1, (5, D))
    return centres[rng.randint(0, 5, n)] + 0.25 * rng.randn(n, D)


class _Stop(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """The library absent: any attempt to reach the device raises _Stop."""
    from phamers_amd import _lib

    def refuse(*a, **k):
        raise _Stop()
    monkeypatch.setattr(_lib, "get_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "Sweep", refuse)
    monkeypatch.delenv("PHAMERS_KMEANS", raising=False)


def test_problem_order_is_k_values_times_seeds(monkeypatch, no_device):
    from phamers_amd import _lib, learning
    seen = {}

    class FakeSweep(object):
        def __init__(self, ctx, X):
            self.n = X.shape[0]

        def run(self, ks, first, draws, silhouettes=True, chunk=0, pair_budget=-1):
            seen["ks"], seen["first"], seen["draws"] = list(ks), list(first), draws
            S = len(ks)
            return {"labels": np.zeros((S, self.n), dtype=np.uint32), "sil": np.tile(np.arange(S, dtype=np.float64)[:, None], (1, self.n)),
                    "status": np.zeros(S, dtype=np.uint32), "n_iter": np.arange(S, dtype=np.int32) + 1,
                    "min_gap": np.ones(S), "seed_margin": np.ones(S), "seeds": [np.zeros(k) for k in ks]}

        def close(self):
            pass

    monkeypatch.setattr(_lib, "get_context", lambda: None)
    monkeypatch.setattr(_lib, "Sweep", FakeSweep)
    X = _blobs(40, 3, 0)
    recs = learning.kmeans_sweep(X, [5, 2, 7], seeds=[10, 11])
    assert [(r["k"], r["seed"]) for r in recs] == [(5, 10), (5, 11), (2, 10), (2, 11), (7, 10), (7, 11)]
    assert seen["ks"] == [5, 5, 2, 2, 7, 7]
    for (k, seed), first, dr in zip([(r["k"], r["seed"]) for r in recs], seen["first"], seen["draws"]):
        f, d = sweep_ref.draws(40, k, seed)
        assert first == f and np.array_equal(dr, d)
    assert [r["n_iter"] for r in recs] == [1, 2, 3, 4, 5, 6] and [r["silhouette"] for r in recs] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    assert all(r["route"] == "device" and r["labels"].dtype == np.int32 for r in recs)
    # without seeds: the reference's seed, one problem per k
    recs = learning.kmeans_sweep(X, np.array([3, 4]))
    assert [(r["k"], r["seed"]) for r in recs] == [(3, learning.kmeans_seed), (4, learning.kmeans_seed)]


def test_argument_errors_come_before_any_device_work(no_device):
    from sklearn.cluster import KMeans
    from sklearn.metrics import silhouette_samples
    from phamers_amd import learning
    X = _blobs(12, 3, 1)
    with pytest.raises(ValueError) as want:
        KMeans(n_clusters=13, random_state=10).fit(X)
    with pytest.raises(ValueError) as got:
        learning.kmeans_sweep(X, [3, 13])
    assert str(got.value) == str(want.value)
    with pytest.raises(ValueError) as got:
        learning.kmeans_sweep(X, [13], silhouettes=False)
    assert str(got.value) == str(want.value)
    for k, labels in ((12, np.arange(12)), (1, np.zeros(12, dtype=int))):
        with pytest.raises(ValueError) as want:
            silhouette_samples(X, labels)
        with pytest.raises(ValueError) as got:
            learning.kmeans_sweep(X, [4, k])
        assert str(got.value) == str(want.value)
    with pytest.raises(ValueError) as want:
        KMeans(n_clusters=0).fit(X)
    with pytest.raises(ValueError) as got:
        learning.kmeans_sweep(X, [0], silhouettes=False)
    assert str(got.value) == str(want.value)
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="Input contains NaN"):
        learning.kmeans_sweep(bad, [3])
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        learning.kmeans_sweep(bad, [3])
    # k = 1 and k = n are fits scikit-learn accepts: without silhouettes they pass the checks and reach the device
    with pytest.raises(_Stop):
        learning.kmeans_sweep(X, [1, 12], silhouettes=False)


def test_gpu_mode_is_not_supported(monkeypatch, no_device):
    from phamers_amd import learning
    monkeypatch.setenv("PHAMERS_KMEANS", "gpu")
    with pytest.raises(NotImplementedError):
        learning.kmeans_sweep(_blobs(12, 3, 1), [3])


def _canned(monkeypatch, values):
    """learning.kmeans_sweep replaced by records whose silhouettes have the given means' bits: (k, seed) -> value."""
    from phamers_amd import learning
    calls = []

    def fake(data, k_values, seeds=None, silhouettes=True, **kw):
        calls.append((list(np.asarray(k_values).tolist()), seeds))
        out = []
        for k in np.asarray(k_values).tolist():
            for seed in ([learning.kmeans_seed] if seeds is None else seeds):
                v = values[(k, seed)]
                out.append({"k": k, "seed": seed, "silhouettes": np.array([v - 0.25, v + 0.25, v]), "silhouette": v,
                            "labels": None, "n_iter": 1, "route": "device"})
        return out
    monkeypatch.setattr(learning, "kmeans_sweep", fake)
    return calls


def test_silhouette_curve_follows_the_reference_arithmetic(monkeypatch):
    from phamers_amd import cluster
    values = {(k, 10): 0.1 * k / 3.0 for k in (2, 3, 5)}
    calls = _canned(monkeypatch, values)
    ks, mean, std = cluster.silhouette_curve(np.zeros((9, 2)), [5, 3, 2, 3], num_repeats=5)
    assert calls == [([2, 3, 5], None)]                       # de-duplicated, sorted, one fit per k
    assert np.array_equal(ks, [2, 3, 5])
    for i, k in enumerate(ks):
        means = np.zeros(5)
        means[:] = np.mean(np.array([values[(k, 10)] - 0.25, values[(k, 10)] + 0.25, values[(k, 10)]]))
        assert mean[i] == np.mean(means) and std[i] == np.std(means)
    # five equal values: 3x and 5x round, so np.mean(means) need not return x nor np.std(means) 0 -- the reference's roundings
    assert np.all(std <= 1e-16) and np.all(np.abs(mean - np.array([np.mean(np.array([v - 0.25, v + 0.25, v])) for v in
                                                                    (values[(2, 10)], values[(3, 10)], values[(5, 10)])])) <= 1e-16)
    # two repeats: x + x and its half are exact
    ks, mean, std = cluster.silhouette_curve(np.zeros((9, 2)), [5, 3, 2], num_repeats=2)
    assert np.all(std == 0.0)
    assert all(mean[i] == np.mean(np.array([values[(k, 10)] - 0.25, values[(k, 10)] + 0.25, values[(k, 10)]])) for i, k in enumerate(ks))
    calls.pop()
    # seeds of its own per repeat
    values = {(k, s): 0.01 * k + 0.001 * s * s for k in (4, 6) for s in (1, 2, 3)}
    calls = _canned(monkeypatch, values)
    ks, mean, std = cluster.silhouette_curve(np.zeros((9, 2)), np.array([6, 4]), num_repeats=3, seeds=[1, 2, 3])
    assert calls == [([4, 6], [1, 2, 3])]
    for i, k in enumerate((4, 6)):
        means = np.array([np.mean(np.array([values[(k, s)] - 0.25, values[(k, s)] + 0.25, values[(k, s)]])) for s in (1, 2, 3)])
        assert mean[i] == np.mean(means) and std[i] == np.std(means) and std[i] > 0
    with pytest.raises(ValueError):
        cluster.silhouette_curve(np.zeros((9, 2)), [4], num_repeats=5, seeds=[1, 2])
    # the default grid is the reference's
    import inspect
    default = inspect.signature(cluster.silhouette_curve).parameters["k_clusters"].default
    assert np.array_equal(default, np.arange(10, 600, 10)) and len(default) == 59


def test_curve_file_layout_and_reading_back(monkeypatch, tmp_path):
    from phamers_amd import cluster, fileIO
    values = {(k, 10): 1.0 / k for k in (2, 4, 6)}
    _canned(monkeypatch, values)
    seen = {}

    def fake_read(path, normalize=False):
        seen["args"] = (path, normalize)
        return np.array(["a", "b"]), np.zeros((9, 4))
    monkeypatch.setattr(fileIO, "read_feature_file", fake_read)
    monkeypatch.chdir(tmp_path)
    assert cluster.main(["-in", "some/dir/phage_features.csv", "--k_clusters", "2", "7", "2", "--repeats", "3"]) == 0
    assert seen["args"] == ("some/dir/phage_features.csv", True)
    path = tmp_path / "phage_features_sil.csv"                   # the reference's default name, .csv for its .svg
    lines = path.read_text().splitlines()
    head = [ln for ln in lines if ln.startswith("#")]
    body = [ln for ln in lines if not ln.startswith("#")]
    assert head[0].startswith("# Silhouette against the number of clusters") and "k,silhouette,std" in head[0]
    assert any(ln.startswith("# features_file:\t") for ln in head) and any(ln.startswith("# repeats:\t3") for ln in head)
    assert len(head) + len(body) == len(lines) and len(body) == 3
    assert [ln.split(",")[0] for ln in body] == ["2", "4", "6"] and all(len(ln.split(",")) == 3 for ln in body)
    ks, mean, std = cluster.read_curve(str(path))
    want = cluster.silhouette_curve(np.zeros((9, 4)), np.arange(2, 7, 2), 3)
    assert np.array_equal(ks, want[0]) and np.array_equal(mean, want[1]) and np.array_equal(std, want[2])   # repr round-trips
    # -out names the file
    assert cluster.main(["-in", "x.csv", "-out", str(tmp_path / "curve.csv"), "--k_clusters", "2", "5", "2"]) == 0
    assert np.array_equal(cluster.read_curve(str(tmp_path / "curve.csv"))[0], [2, 4])


def test_restatement_against_scikit_learn():
    from sklearn.cluster import KMeans
    from sklearn.metrics import silhouette_samples
    X = _blobs(150, 9, 5)
    for k, seed in ((2, 10), (4, 10), (9, 11), (40, 10)):
        ref = sweep_ref.kmeans(X, k, seed)
        fit = KMeans(n_clusters=k, random_state=seed).fit(X)
        print(k, seed, "margin %.3g gap %.3g empty %d" % (ref["seed_margin"], ref["min_gap"], ref["n_empty"]))
        assert ref["seed_margin"] >= 1e-8 and ref["min_gap"] >= 1e-7 and ref["n_empty"] == 0   # (else the case proves nothing)
        assert np.array_equal(ref["labels"], fit.labels_) and ref["n_iter"] == fit.n_iter_
        assert np.max(np.abs(sweep_ref.silhouettes(X, ref["labels"]) - silhouette_samples(X, fit.labels_))) <= 1e-8
        from phamers_amd import learning
        assert np.array_equal(ref["seeds"], learning.kmeans_plusplus_seeds(sweep_ref.centre(X), k, np.random.RandomState(seed))[1])
