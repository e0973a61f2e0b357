"""The NumPy restatement of the embedding (tests/manifold_ref.py) against scikit-learn, stage by stage, so that the GPU tests
can hold the device to the restatement; the t-SNE file format; phamer_scorer's attributes; what is refused.  No GPU."""
import os

import numpy as np
import pytest
from scipy.spatial.distance import squareform

from tests import manifold_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "manifold.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def small():
    X = ref.reference_rows(GOLDEN, 100)
    Z = ref.pca(X, 20)[0]
    k = min(X.shape[0] - 1, int(3 * 12.0 + 1))
    idx, d2 = ref.neighbors(Z, k)
    P, beta = ref.binary_search_perplexity(d2, 12.0)
    return dict(X=X, Z=Z, k=k, idx=idx, d2=d2, P=P, csr=ref.symmetrize(idx, P))


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def test_fma_emulation_is_exact():
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a, b, c = rng.standard_normal(2000), rng.standard_normal(2000), rng.standard_normal(2000) * 1e-3
    c[:500] = -(a[:500] * b[:500])    # cancellation: the product's low part decides
    got = ref.fma(a, b, c)
    for i in range(2000):
        exact = Fraction(a[i]) * Fraction(b[i]) + Fraction(c[i])
        assert got[i] == float(exact), i    # float(Fraction) rounds correctly


def test_pca_is_scikit_learns_full_solver(small):
    from sklearn.decomposition import PCA
    sk = PCA(n_components=20, svd_solver="full")
    T = sk.fit_transform(small["X"])
    Tr, comps, mean, var = ref.pca(small["X"], 20)
    assert rel(Tr, T) < 1e-10 and rel(comps, sk.components_) < 1e-8
    assert rel(mean, sk.mean_) < 1e-14 and rel(var, sk.explained_variance_) < 1e-10


def test_joint_probabilities_are_scikit_learns(small):
    from sklearn.manifold import _t_sne
    from sklearn.neighbors import NearestNeighbors
    n, k = small["Z"].shape[0], small["k"]
    g = NearestNeighbors(n_neighbors=k).fit(small["Z"]).kneighbors_graph(mode="distance")
    g.data **= 2
    g.sort_indices()
    # a neighbourhood edge that is a tie between identical distances (duplicate rows) is decided by index here and
    # arbitrarily by scikit-learn: the sets are compared on the other rows, and the search runs on this side's graph
    d2x = ref.neighbors(small["Z"], k + 1)[1]
    clear = d2x[:, k] > d2x[:, k - 1]
    assert clear.sum() >= 0.9 * n
    assert np.array_equal(np.sort(small["idx"], axis=1)[clear], g.indices.reshape(n, k)[clear])
    assert rel(np.sort(small["d2"], axis=1)[clear], np.sort(g.data.reshape(n, k), axis=1)[clear]) < 1e-12
    from scipy.sparse import csr_matrix
    by_col = np.argsort(small["idx"], axis=1)
    g = csr_matrix((np.take_along_axis(small["d2"], by_col, axis=1).ravel(), np.sort(small["idx"], axis=1).ravel(),
                    np.arange(0, n * k + 1, k)), shape=(n, n))
    P_sk = _t_sne._joint_probabilities_nn(g, 12.0, 0).toarray()
    # scikit-learn searches on float32 distances: the documented difference, a few 1e-7 of the largest entry
    assert rel(ref.dense(small["csr"]), P_sk) < 5e-6
    assert abs(small["csr"][2].sum() - 1.0) < 1e-12


def test_objective_and_gradient_are_scikit_learns_float64(small):
    from sklearn.manifold import _t_sne
    n = small["Z"].shape[0]
    Pc = squareform(ref.dense(small["csr"]), checks=False)
    rng = np.random.default_rng(1)
    for scale in (1e-4, 1.0, 30.0):
        Y = scale * rng.standard_normal((n, 2))
        kl_sk, g_sk = _t_sne._kl_divergence(Y.ravel().copy(), Pc, 1.0, n, 2)
        kl, g = ref.kl_gradient(Y, small["csr"])
        assert abs(kl - kl_sk) <= 1e-12 * abs(kl_sk) and rel(g.ravel(), g_sk) < 1e-11


def test_descent_is_scikit_learns(small):
    from sklearn.manifold import _t_sne
    n = small["Z"].shape[0]
    Pc = squareform(ref.dense(small["csr"]), checks=False)
    Y0 = small["Z"][:, :2] / np.std(small["Z"][:, 0]) * 1e-4
    p_sk, _, _ = _t_sne._gradient_descent(_t_sne._kl_divergence, Y0.ravel().copy(), 0, 10, n_iter_check=10 ** 9, momentum=0.5,
                                          learning_rate=50.0, args=[Pc * 12.0, 1.0, n, 2])
    Y = ref.descend(Y0, small["csr"], 10, exaggeration=12.0, momentum=0.5, learning_rate=50.0)
    # (ten steps: the iteration amplifies rounding -- the fixture records 4e-13, 4e-10 and 2e-5 of the span after 10, 50, 250)
    assert np.max(np.abs(Y.ravel() - p_sk)) <= 1e-9 * np.ptp(p_sk)
    # the control loop: checks every 50 iterations, both phases
    Y, kl, it = ref.tsne(Y0, small["csr"], 12.0, 200.0, max_iter=300)
    assert it == 299 and abs(kl - ref.kl_gradient(ref.tsne(Y0, small["csr"], 12.0, 200.0, max_iter=299)[0], small["csr"])[0]) \
        <= 1e-12 * abs(kl)      # the reported error is the objective BEFORE the last update


def test_trustworthiness_is_scikit_learns(small):
    from sklearn.manifold import trustworthiness
    Y = np.random.default_rng(2).standard_normal((small["Z"].shape[0], 2)) + small["Z"][:, :2] * 50
    # (duplicate rows in Z: their rank ties fall differently in scikit-learn's Gram-form distances)
    assert abs(ref.trustworthiness(small["Z"], Y, 12) - trustworthiness(small["Z"], Y, n_neighbors=12)) < 1e-3
    Zu = np.random.default_rng(3).standard_normal((150, 5))
    Yu = Zu[:, :2] + 0.3 * np.random.default_rng(4).standard_normal((150, 2))
    assert abs(ref.trustworthiness(Zu, Yu, 12) - trustworthiness(Zu, Yu, n_neighbors=12)) < 1e-12


def test_fixture_records_what_the_tests_need(gold):
    for key in ("versions", "pca_dev_transformed", "pca_dev_components", "cond_dev", "cond_dev_f32", "joint_dev", "kl_dev",
                "grad_dev", "traj_steps", "traj_dev", "final_kl", "final_trust", "Y_mid", "Y_end"):
        assert key in gold, key
    assert len(gold["final_kl"]) == 6 and list(gold["traj_steps"]) == [10, 50, 250]
    # the float64 figures are rounding-sized; the float32-distance figure is what the documented difference costs
    assert gold["cond_dev"] < 1e-9 and gold["grad_dev"] < 1e-9 and gold["cond_dev_f32"] < 1e-4


def test_tsne_file_format(gold, tmp_path):
    from phamers_amd import fileIO
    pts = gold["tsne_file_points"]
    ids = [str(i) for i in gold["tsne_file_ids"]]
    path = str(tmp_path / "tsne_coordinates.csv")
    fileIO.save_tsne_data(path, pts, ids, chops=(2, 2, 1))
    with open(path) as f:
        assert f.read() == str(gold["tsne_file_text"])      # what the reference's own save_tsne_data wrote
    got_ids, got_pts, chops = fileIO.read_tsne_file(path)
    assert got_ids == ids and np.array_equal(got_pts, pts) and chops == [2, 2, 1]
    fileIO.save_tsne_data(path, pts, ids)
    assert fileIO.read_tsne_file(path)[2] is None
    with pytest.raises(ValueError):
        fileIO.read_tsne_file(None)


def test_scorer_attributes_are_the_references():
    from phamers_amd import phamer
    s = phamer.phamer_scorer()
    assert s.tsne_perplexity == 30.0 and s.early_exaggeration == 1.0 and s.tsne_init == "pca"
    assert s.tsne_learning_rate == 2000 and s.tsne_seed == 10 and s.pca_preprocess is True and s.pca_preprocess_red == 50
    assert s.tsne_data is None
    s.output_directory = "out"
    assert s.get_tsne_output_filename() == os.path.join("out", "tsne_coordinates.csv")
    assert not hasattr(s, "use_tsne_python")


def test_what_is_refused():
    from phamers_amd import manifold
    X = np.zeros((10, 3))
    for kw in (dict(n_components=3), dict(metric="cosine"), dict(method="exact")):
        with pytest.raises(NotImplementedError):
            manifold.TSNE(perplexity=2, **kw).fit_transform(X)
    with pytest.raises(ValueError, match="perplexity must be less than n_samples"):
        manifold.TSNE(perplexity=10).fit_transform(X)
    bad = X.copy()
    bad[0, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        manifold.PCA(2).fit_transform(bad)
    t = manifold.TSNE()
    assert (t.perplexity, t.early_exaggeration, t.learning_rate, t.max_iter, t.n_iter_without_progress, t.min_grad_norm,
            t.init, t.method, t.angle) == (30.0, 12.0, 'auto', 1000, 300, 1e-7, 'pca', 'barnes_hut', 0.5)


# ---- conditions on the inputs and references of tests/test_gpu_manifold_shapes.py ---------------------------------------
@pytest.mark.parametrize("seed,n,side,d,k", ref.LATTICE_CASES)
def test_lattice_cases_cut_a_class_of_hundreds_of_equal_distances(seed, n, side, d, k):
    """Some row's threshold class has more than 256 members and is cut inside; the taken members span several 256-entry
    scan steps, and in the cut's own step members of an earlier wave precede it."""
    Z = ref.lattice_rows(seed, n, side, d)
    assert n % 64 != 0
    D = ref.sqdist_rows(Z, np.arange(n))
    assert np.array_equal(D, np.round(D))
    D[np.arange(n), np.arange(n)] = np.inf
    big = steps = waves = 0
    for i in range(n):
        members, need = ref.tie_cut(D[i], k)
        if len(members) > 256 and 0 < need < len(members):
            taken, cut = members[:need], members[need - 1]
            big += 1
            steps += bool(members[0] // 256 < cut // 256)
            waves += bool(np.any((taken // 256 == cut // 256) & ((taken % 256) // 64 < (cut % 256) // 64)))
    assert big >= 100 and steps >= 100 and waves >= 100, (big, steps, waves)


def test_affinity_edge_cases_keep_their_rows():
    """At least 95% of each case's rows stop with a margin >= 1e-9 to the 1e-5 threshold at every step; the scaled cases
    take the branches they are there for."""
    for name, d2, perplexity in ref.affinity_edge_cases():
        P, beta, margin = ref.binary_search_perplexity(d2, perplexity, margins=True)
        assert np.mean(margin >= 1e-9) >= 0.95, name
        assert np.allclose(P.sum(axis=1), 1.0, rtol=1e-12), name
    cases = {name: d2 for name, d2, _ in ref.affinity_edge_cases()}
    assert np.exp(-cases["x1e6"]).max() == 0.0          # sum_p == 0 at beta = 1
    assert ref.binary_search_perplexity(cases["x1e6"][:8], 30.0)[1].max() < 1e-5      # ... halved ~19 times
    assert ref.binary_search_perplexity(cases["x1e-6"][:8], 30.0)[1].min() > 1e5      # doubled ~20 times
    P, beta = ref.binary_search_perplexity(np.zeros((2, 40)), 5.0)
    assert np.all(beta == 2.0 ** 100) and np.all(P == 1.0 / 40)


@pytest.mark.parametrize("name", sorted(ref.CONTROL_CASES))
def test_control_cases_decide_with_a_margin(name):
    """Every decision of every control-loop case has a relative margin >= 1e-6 on the reference side, and the case ends
    where it was chosen to end."""
    log = []
    Y, kl, it = ref.control_reference(name, log)
    kw = ref.CONTROL_CASES[name]
    assert it == ref.CONTROL_EXPECTED_N_ITER[name]
    assert ref.decision_margins(log, moved=kw["learning_rate"] > 0) >= 1e-6
    if name == "max_iter_250":
        assert kl == np.finfo(float).max and not [l for l in log if l[0] > 249]
    if name == "grad_norm_phase_1":        # stopped at the first check of each phase: phase 2 began at it + 1 = 50
        assert [l[0] for l in log] == [49, 99]
    if name == "grad_norm_phase_2":        # phase 1 ran through, phase 2 stopped at its first check
        assert [l[0] for l in log] == [49, 99, 149, 199, 249, 299] and log[-1][3] <= kw["min_grad_norm"] < log[-2][3]
    if name == "stall":                    # 349: j - best_iter == limit, not an improvement, goes on; 399: stops
        assert [(l[0], l[4]) for l in log if l[0] > 249] == [(299, 0), (349, 50), (399, 100)] and log[-1][5] == 50
        assert log[-2][1] == log[-2][2]


def test_one_pass_covariance_misses_the_bound_the_device_is_held_to():
    n, D, offset = ref.PCA_CASES[-1]
    assert offset == 1e6
    X = ref.spectrum_data(n, n, D, offset)
    mean, cov, gram = ref.covariance(X)
    bound, chain = ref.covariance_bound(n, D, gram)
    two_pass = (X - X.mean(axis=0)).T @ (X - X.mean(axis=0)) / (n - 1)
    assert np.all(np.abs(two_pass - cov) <= bound)                     # float64, two passes: inside
    err = np.abs(ref.covariance_one_pass(X) - cov).astype(np.float64)
    assert np.max(err / bound) > 100.0                                  # float64, one pass: far outside


def test_chunk_rows_of_the_cap_case():
    n, D = ref.PCA_CAP_CASE
    assert ref.pca_chunk_rows(n, D) == 1052 > 1024 and ref.pca_chunk_rows(n, 2048) == 1024
    assert n * D * 8 < 80e6 and (n - 1052) % 4 != 0
    assert ref.pca_chunk_rows(2049, 257) == 1024 and ref.pca_chunk_rows(5000, 300) == 1024


def test_lattice_reference_is_the_pairwise_one():
    n = 3000
    Y, cells, counts = ref.lattice_embedding(41, n, 16)
    csr = ref.ring_csr(n, 42)
    assert counts.max() > 1 and np.all(np.diff(csr[0]) >= 2) and abs(csr[2].sum() - 1.0) < 1e-12
    rows = np.array([0, 1, 255, 256, 1500, n - 1])
    kl, g, Z, rep_abs, att_abs, kl_abs = ref.kl_gradient_lattice(Y, cells, counts, csr, rows)
    kl_r, g_r = ref.kl_gradient(Y, csr, rows=rows)
    assert abs(float(kl) - kl_r) <= 1e-12 * abs(kl_r)
    assert rel(g.astype(np.float64), g_r) < 1e-11
    assert rep_abs.shape == att_abs.shape == (len(rows), 2) and kl_abs >= abs(kl)
    assert ref.gradient_ranges(11521)[:2] == (46, 45) and ref.gradient_ranges(20000)[:2] == (79, 26)
    assert ref.gradient_ranges(524288 + 257)[:2] == (2050, 1) and ref.gradient_ranges(8448)[:2] == (33, 33)


def test_perplexity_above_the_sort_width_never_reaches_the_device(monkeypatch):
    from phamers_amd import manifold

    def no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(manifold._lib, "get_context", no_device)
    X = ref.synthetic(3, 4200, 2)
    with pytest.raises(ValueError, match="k=4097 neighbours"):
        manifold.neighbors(X, 4097)
    with pytest.raises(ValueError, match="k=4099 neighbours: must be between 1 and min"):
        manifold.TSNE(perplexity=1366).fit_transform(X)
