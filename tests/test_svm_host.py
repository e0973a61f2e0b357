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


# ---- synthetic dyadic cases (tests/golden/scoring_svm_synth.npz, tools/gen_golden_svm_synth.py) --------------------------
SYNTH_CASES = ("long", "maxiter", "shrink")
SYNTH_DATA = {"long": "long", "maxiter": "long", "shrink": "shrink"}
EXACT = 1e-12


def synth_case(s, case):
    """(train rows, labels, queries, nu, max_iter) of a synthetic case; every entry a multiple of 2^-12."""
    ds = SYNTH_DATA[case]
    u = float(s["unit"])
    return (s["X_" + ds] / u, s["y_" + ds].astype(np.float64), s["q_" + ds] / u, float(s["nu_" + case]),
            int(s["max_iter_" + case]))


@pytest.fixture(scope="module")
def synth():
    return helpers.load_npz("scoring_svm_synth.npz")


_REF_FITS = {}


def synth_ref_fit(s, case):
    """svm_ref.Fit of a synthetic case with its TAU counters (cached: the long case takes a few seconds)."""
    if case not in _REF_FITS:
        X, y, _, nu, max_iter = synth_case(s, case)
        cnt = {}
        f = svm_ref.Fit(X, y, nu=nu, max_iter=max_iter, counters=cnt)
        _REF_FITS[case] = (f, cnt)
    return _REF_FITS[case]


@pytest.mark.parametrize("case", SYNTH_CASES)
def test_restatement_reproduces_the_unshrunk_synthetic_fits(synth, case):
    """svm_ref.Fit against NuSVC(shrinking=False) on dyadic data: the same iterations and support vectors, coefficients and
    intercept within 1e-12, decisions within 1e-9 (plus the cancellation term), predictions exact."""
    s, t = synth, case + "_noshrink"
    X, y, q, _, _ = synth_case(s, case)
    f = synth_ref_fit(s, case)[0]
    assert f._gamma == float(s["gamma_" + t])
    assert int(f.n_iter_[0]) == int(s["n_iter_" + t][0])
    assert np.array_equal(f.support_, s["support_" + t])
    assert np.max(np.abs(f.dual_coef_[0] - s["dual_coef_" + t])) <= EXACT
    assert abs(f.intercept_[0] - s["intercept_" + t][0]) <= EXACT
    assert np.max(np.abs(f.decision_function(q) - s["dec_" + t])) <= dec_tol(s, t, 1e-9)
    assert np.array_equal(f.predict(q), s["pred_" + t].astype(np.float64))


def test_synthetic_fixture_shapes(synth):
    """The long case needs three launches of the GPU solver (4 096 iterations each) and leaves room for max_iter = 8 193;
    max_iter = 4 097 stops there; the generator refused near-zero decisions."""
    s = synth
    assert int(s["n_iter_long_noshrink"][0]) > 2 * 4096 + 1
    assert int(s["n_iter_maxiter_noshrink"][0]) == int(s["max_iter_maxiter"]) == 4097
    for t in [c + "_" + m for c in SYNTH_CASES for m in ("noshrink", "default")]:
        assert np.abs(s["dec_" + t]).min() >= 1e-5, t
    X = s["X_long"]
    y = s["y_long"]
    assert np.array_equal(X[0], X[1]) and y[0] == y[1]
    assert np.array_equal(X[2], X[3]) and y[2] != y[3]


def test_shrinking_changes_the_solution_in_general(synth):
    """What DESIGN.md and phamers_amd/svm.py state: scikit-learn's NuSVC() (shrinking on) and NuSVC(shrinking=False) can
    end at different solutions.  On the 'shrink' case they differ in iterations, intercept and some predictions; on the
    long case they agree."""
    s = synth
    a, b = "shrink_noshrink", "shrink_default"
    assert int(s["n_iter_" + a][0]) != int(s["n_iter_" + b][0])
    assert abs(s["intercept_" + a][0] - s["intercept_" + b][0]) > 1e-5
    assert (s["pred_" + a] != s["pred_" + b]).any()
    a, b = "long_noshrink", "long_default"
    assert int(s["n_iter_" + a][0]) == int(s["n_iter_" + b][0])
    assert np.array_equal(s["support_" + a], s["support_" + b])
    assert np.array_equal(s["pred_" + a], s["pred_" + b])


def test_long_case_takes_the_tau_branches(synth):
    """libsvm's quad_coef <= 0 -> TAU branches on the long case: in the choice of j and in the update of a same-label pair
    (near duplicates: Q_ij rounds to 1.0f while the gradients differ).  Exact duplicates never reach them (their gradients
    stay equal, so grad_diff = 0), and Solver_NU never updates a pair of opposite labels."""
    s = synth
    cnt = synth_ref_fit(s, "long")[1]
    assert cnt["tau_j"] >= 1
    assert cnt["tau_same"] >= 1
    assert cnt["tau_opposite"] == 0
    # the near-duplicate rows are what makes quad_coef vanish: Q_ij = 1.0f with x_i != x_j
    X, y, _, _, _ = synth_case(s, "long")
    perm, yg = svm_ref.grouped_order(y)
    Q = svm_ref.kernel_matrix(X[perm[:64]], yg[:64], svm_ref.gamma_scale(X))
    pos = {p: k for k, p in enumerate(perm[:64])}
    pairs = [(i, j) for i in pos for j in pos
             if i < j and y[i] == y[j] and not np.array_equal(X[i], X[j]) and Q[pos[i], pos[j]] == 1.0]
    assert pairs


def test_max_iter_stops_the_restatement(synth):
    X, y, _, nu, _ = synth_case(synth, "long")
    perm, yg = svm_ref.grouped_order(y)
    Q = svm_ref.kernel_matrix(X[perm], yg, svm_ref.gamma_scale(X))
    for m in (1, 2, 5000):
        assert svm_ref.solve_nu(Q, yg, nu, 1e-3, m)[4] == m


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
