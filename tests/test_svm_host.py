"""CPU: the svm and dbscan methods' fixture, its NumPy restatement and the host-side rules, without a device."""
import numpy as np
import pytest

from tests import helpers, svm_ref

TOL = 1e-9
SVM_CASES = ("full", "eq", "auto", "fold0", "fold1", "k5")


def dec_tol(g, tag, tol):
    """tol, plus 1e-14 of the sum of |dual_coef| -- the size of the terms a decision value cancels: on the 'auto' case
    (gamma = 1/256, a smooth kernel) the coefficients reach 7e3 and sum to 1.6e7 for values of order 1."""
    return tol + 1e-14 * float(np.abs(g["dual_coef_" + tag]).sum())


def _ref_matrices():
    from oracle import oracle
    ref = helpers.load_npz("ref_features.npz")
    return (oracle.normalize_counts(ref["pos_counts"].astype(np.int64)),
            oracle.normalize_counts(ref["neg_counts"].astype(np.int64)))


def svm_case(g, tag):
    """(train rows, labels, queries, gamma argument) of a fixture case, rebuilt from the fixtures that hold the inputs."""
    if tag == "k5":
        h = helpers.load_npz("scoring_highdim.npz")
        pos, neg, q = h["pos_k5"], h["neg_k5"], h["q_k5"]
    else:
        pos, neg = _ref_matrices()
        if tag.startswith("fold"):
            f = int(tag[4:])
            pa, na = g["cv_pos_asmt"], g["cv_neg_asmt"]
            q = np.vstack((pos[pa == f], neg[na == f]))
            pos, neg = pos[pa != f], neg[na != f]
        else:
            q = np.vstack((helpers.load_npz("scoring_k4.npz")["q"], g["mix_q"]))
            if tag in ("eq", "auto"):
                m = int(g["n_equalized"][0])
                pos, neg = pos[:m], neg[:m]
    X = np.vstack((pos, neg))
    y = np.append(np.ones(len(pos)), np.zeros(len(neg)))
    return X, y, q, ("auto" if tag == "auto" else "scale")


@pytest.fixture(scope="module")
def golden():
    return helpers.load_npz("scoring_svm.npz")


@pytest.mark.parametrize("tag", SVM_CASES)
def test_restatement_reproduces_scikit_learn(golden, tag):
    """tests/svm_ref.py (libsvm's Solver_NU without shrinking, float32 Q) against the stored scikit-learn fit: the same
    iterations and support vectors, coefficients and decisions within 1e-9, the same predictions."""
    g = golden
    X, y, q, gamma = svm_case(g, tag)
    f = svm_ref.Fit(X, y, gamma=gamma)
    assert f._gamma == float(g["gamma_" + tag])
    assert int(f.n_iter_[0]) == int(g["n_iter_" + tag][0])
    assert np.array_equal(f.support_, g["support_" + tag])
    assert np.max(np.abs(f.dual_coef_[0] - g["dual_coef_" + tag])) <= TOL
    assert abs(f.intercept_[0] - g["intercept_" + tag][0]) <= TOL
    dec = f.decision_function(q)
    assert np.max(np.abs(dec - g["dec_" + tag])) <= dec_tol(g, tag, TOL)
    assert np.array_equal(f.predict(q), g["pred_" + tag])


def test_full_matrix_figures(golden):
    """What the issue's scratch check found on the whole reference: 1 278 iterations, 2 358 support vectors, gamma ~ 555."""
    assert int(golden["n_iter_full"][0]) == 1278
    assert len(golden["support_full"]) == 2358
    assert abs(float(golden["gamma_full"]) - 554.77) < 0.01
    for tag in SVM_CASES:        # the generator refused near-zero decisions
        assert np.abs(golden["dec_" + tag]).min() >= 1e-5


@pytest.mark.parametrize("tag", ("full", "eq", "fold0", "k5"))
def test_gamma_scale_has_scikit_learns_bits(golden, tag):
    from phamers_amd import _lib
    X = svm_case(golden, tag)[0]
    assert _lib.svm_gamma(X, "scale") == float(golden["gamma_" + tag])
    assert svm_ref.gamma_scale(X) == float(golden["gamma_" + tag])
    assert _lib.svm_gamma(X, "auto") == 1.0 / X.shape[1]
    assert _lib.svm_gamma(np.ones((4, 3)), "scale") == 1.0      # zero variance
    for bad in ("other", 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _lib.svm_gamma(X, bad)


def test_nu_infeasible_and_single_class_errors():
    """svm_check_parameter's rule (nu (n0 + n1) / 2 > min(n0, n1)) and the single-class refusal, as scikit-learn raises them;
    phamers_amd.svm.NuSVC raises them before it needs a device."""
    from phamers_amd import svm
    rng = np.random.RandomState(0)
    X = rng.rand(40, 8)
    y = np.r_[np.ones(10), np.zeros(30)]          # nu = 0.5: 0.5 * 40 / 2 = 10 <= 10 feasible; 0.6: 12 > 10
    assert svm_ref.check_nu(0.5, 30, 10) is None
    assert svm_ref.check_nu(0.6, 30, 10) == "specified nu is infeasible"
    with pytest.raises(ValueError, match="specified nu is infeasible"):
        svm_ref.Fit(X, y, nu=0.6)
    with pytest.raises(ValueError, match="specified nu is infeasible"):
        svm.NuSVC(nu=0.6).fit(X, y)
    with pytest.raises(ValueError, match="nu <= 0 or nu > 1"):
        svm.NuSVC(nu=1.5).fit(X, y)
    with pytest.raises(ValueError, match="greater than one"):
        svm.NuSVC().fit(X, np.ones(40))
    with pytest.raises(ValueError, match="greater than one"):
        svm_ref.Fit(X, np.ones(40))
    with pytest.raises(NotImplementedError):
        svm.NuSVC(kernel="linear")
    with pytest.raises(NotImplementedError):
        svm.NuSVC(probability=True)
    with pytest.raises(NotImplementedError):
        svm.NuSVC().fit(X, y, sample_weight=np.ones(40))
    with pytest.raises(NotImplementedError):
        svm.NuSVC().fit(X, np.arange(40) % 3)


def _proximity_scores(q, cpos, cneg):
    """phamer_scorer.proximity_metric with learning.closest_to (first index of the smallest distance)."""
    out = np.empty(len(q))
    for i, p in enumerate(q):
        cp = cpos[np.argmin(np.sqrt(((cpos - p) ** 2).sum(1)))]
        cn = cneg[np.argmin(np.sqrt(((cneg - p) ** 2).sum(1)))]
        ep, en = np.linalg.norm(p - cp), np.linalg.norm(p - cn)
        out[i] = np.tanh((en - ep) / (ep + en))
    return out


@pytest.mark.parametrize("tag,fallback", (("default", (True, True)), ("eps0", (False, False)), ("eps1", (False, True))))
def test_dbscan_fixture_follows_the_restated_control_flow(golden, tag, fallback):
    """scripts/phamer.py:212-238 restated on the stored labels: k-means where DBSCAN's largest label is < 2, the clusters'
    means without the noise points, the proximity metric; shape (n, 1)."""
    g = golden
    pos, neg = _ref_matrices()
    q = helpers.load_npz("scoring_k4.npz")["q"]
    cents = []
    for cls, data, fb in (("pos", pos, fallback[0]), ("neg", neg, fallback[1])):
        a = g["dbscan_%s_labels_%s" % (cls, tag)].astype(np.int64)
        assert (a.max() < 2) == fb
        if fb:
            a = g["dbscan_%s_kmeans_%s" % (cls, tag)].astype(np.int64)
        elif tag == "eps0":
            assert (a == -1).any() and a.max() >= 2       # many clusters and some noise
        cents.append(np.array([data[a == c].mean(axis=0) for c in sorted(set(a.tolist()) - {-1})]))
    want = g["dbscan_" + tag]
    assert want.shape == (len(q), 1)
    got = _proximity_scores(q, *cents)
    assert np.max(np.abs(got - want[:, 0])) <= 1e-12


def test_method_table():
    """svm and dbscan are scoring methods now; silhouette still raises, with the reason."""
    from phamers_amd import phamer
    sc = phamer.phamer_scorer()
    for m in ("dbscan", "svm"):
        assert sc.method_function_map[m] == getattr(sc, m + "_score_points")
    assert (sc.eps, sc.min_samples, sc.k_clusters_positive, sc.k_clusters_negative) == ([1, 1], [2, 2], 86, 20)
    sc.scoring_method = "silhouette"
    sc.data_points = np.zeros((2, 256))
    sc.positive_data = sc.negative_data = np.zeros((2, 256))
    with pytest.raises(NotImplementedError, match="positive data twice"):
        sc.score_points()
