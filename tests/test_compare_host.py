"""CPU only: the statement tests/compare_ref.py against independent sources (scipy's midranks and Mann-Whitney U, the integer
ROC method, np.cov), its own two bootstrap forms against each other, and the checks phamers_amd/compare.py makes before any
device work.  No device is touched: the module's refusals are raised before a context is asked for."""
import numpy as np
import pytest
from scipy import stats

from tests import compare_ref as ref
from tests import evaluate_ref

P, N = 37, 45


@pytest.fixture(scope="module")
def scores():
    return ref.noisy_cells(np.random.RandomState(3), P, N, 5)   # three noisy cells with ties, a +-1 cell, a duplicate of cell 0


def test_placements_are_midrank_differences_and_sum_to_the_area(scores):
    t_pos, t_neg = ref.placements(scores, P)
    for c, row in enumerate(scores):
        pos, neg = row[:P], row[P:]
        assert np.array_equal(t_pos[c], 2 * (stats.rankdata(row)[:P] - stats.rankdata(pos)))
        assert np.array_equal(2 * P - t_neg[c], 2 * (stats.rankdata(row)[P:] - stats.rankdata(neg)))   # (by symmetry)
        labels = np.r_[np.ones(P, np.uint8), np.zeros(N, np.uint8)]
        area2 = evaluate_ref.roc_points(row, labels)[3]
        assert int(t_pos[c].sum()) == area2 == int(t_neg[c].sum())
        assert area2 == 2 * stats.mannwhitneyu(pos, neg).statistic


def test_covariance_agrees_with_the_float_form(scores):
    st = ref.Statement(scores, P)
    V10, V01 = st.t_pos / (2.0 * N), st.t_neg / (2.0 * P)
    want = np.cov(V10) / P + np.cov(V01) / N
    got = st.covariance()
    assert np.array_equal(got, got.T)
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    assert np.array_equal(st.auc(), [evaluate_ref.rates(*(evaluate_ref.roc_points(
        row, np.r_[np.ones(P, np.uint8), np.zeros(N, np.uint8)])[i] for i in (0, 1, 3)))[2] for row in scores])


def test_a_duplicated_cell_has_no_variance_of_the_difference(scores):
    st = ref.Statement(scores, P)
    assert np.array_equal(scores[0], scores[4])
    assert st.delta(0, 4) == 0.0 and st.delta_variance(0, 4) == 0.0
    assert np.isnan(st.z(0, 4)) and np.isnan(st.p_value(0, 4))
    assert st.delta_variance(0, 1) > 0.0 and 0.0 <= st.p_value(0, 1) <= 1.0
    assert st.z(0, 1) == -st.z(1, 0)


def test_weights_sum_to_the_class_sizes_and_depend_on_seed_and_resample_only():
    for seed in (0, 2 ** 63 + 5):
        w = [ref.weights(seed, b, P, N) for b in range(6)]
        for v in w:
            assert v[:P].sum() == P and v[P:].sum() == N and v.min() >= 0
        assert any(not np.array_equal(w[0], v) for v in w[1:])
    assert not np.array_equal(ref.weights(0, 1, P, N), ref.weights(1, 1, P, N))
    # the rule in Python integers, draw by draw
    key = ref.splitmix64(ref.splitmix64(7) ^ (2 * 3 + 1))
    assert ref.draws(7, 3, 1, N).tolist() == [(ref.splitmix64((key + t) & ref.MASK) * N) >> 64 for t in range(N)]


def test_run_formula_equals_brute_force(scores):
    tied = np.vstack((scores, np.full(P + N, 0.25), np.r_[np.zeros(P), -np.zeros(N)]))   # + one run; +0.0 against -0.0
    brute = ref.bootstrap_brute(tied, P, 11, 4)
    assert np.array_equal(brute, ref.bootstrap_runs(tied, P, 11, 4))
    assert np.all(brute[:, 5] == P * N) and np.all(brute[:, 6] == P * N) and np.all(brute <= 2 * P * N)
    # the draws do not change with B: resample b is a function of (seed, b)
    assert np.array_equal(ref.bootstrap_brute(tied, P, 11, 2, first=2), brute[2:])
    assert np.array_equal(ref.bootstrap_runs(tied, P, 11, 1), brute[:1])
    # unit weights give the area itself
    st = ref.Statement(tied, P)
    assert [int(v) for v in st.t_pos.sum(axis=1)] == st.area2


def _assert_sort_forms_equal_brute_force(m, n_pos):
    t_pos, t_neg = ref.placements(m, n_pos)
    s_pos, s_neg = ref.placements_by_sort(m, n_pos)
    assert s_pos.dtype == np.int64 and np.array_equal(s_pos, t_pos) and np.array_equal(s_neg, t_neg)
    area2, g10, g01 = ref.grams(t_pos, t_neg)
    e_area2, e10, e01 = ref.grams_exact(s_pos, s_neg)
    assert e_area2 == area2 and all(type(a) is int for a in e_area2)
    assert e10.dtype == object and np.array_equal(e10, g10) and np.array_equal(e01, g01)
    assert all(type(v) is int for v in e10.ravel()) and all(type(v) is int for v in e01.ravel())


@pytest.mark.parametrize("name", sorted(evaluate_ref.cases()))
def test_sort_based_placements_and_chunked_grams_equal_brute_force_on_the_cases(name):
    pos, neg = evaluate_ref.cases()[name]
    _assert_sort_forms_equal_brute_force(np.concatenate((pos, neg))[None, :], len(pos))


@pytest.mark.parametrize("shape", [(37, 45), (301, 212)], ids=lambda s: "%dx%d" % s)
def test_sort_based_placements_and_chunked_grams_equal_brute_force_on_noisy_cells(shape, monkeypatch):
    p, n = shape
    m = ref.noisy_cells(np.random.RandomState(p), p, n, 6)
    a, b = evaluate_ref.cases()["rounded"]                 # holds +0.0 and -0.0 in both classes
    signed = np.r_[a[:p], b[:n]]
    assert np.signbit(signed[signed == 0]).any() and not np.signbit(signed[signed == 0]).all()
    assert (signed[:p] == 0).any() and (signed[p:] == 0).any()
    m = np.vstack((m, signed))
    _assert_sort_forms_equal_brute_force(m, p)
    st, by_sort = ref.Statement(m, p), ref.Statement(m, p, by_sort=True)
    assert by_sort.area2 == st.area2 and np.array_equal(by_sort.covariance(), st.covariance())
    monkeypatch.setattr(ref, "GRAM_CHUNK", 64)             # several chunks and a partial last one
    _assert_sort_forms_equal_brute_force(m, p)


def test_chunked_grams_are_exact_where_int64_is_not():
    """Placements of the size the device meets at its limit (below 2^23), enough rows for a sum past 2^63: the chunked form
    equals Python-integer arithmetic, and the uint64 dot product (mod 2^64) agrees with it below 2^64."""
    rng = np.random.RandomState(1)
    rows = ref.GRAM_CHUNK + ref.GRAM_CHUNK // 2 + 11        # two chunks; rows 2^46 lies between 2^63 and 2^64
    t = rng.randint(2 ** 23 - 4096, 2 ** 23, (2, rows)).astype(np.int64)
    area2, g, _ = ref.grams_exact(t, t[:, :5])
    want = [[sum(int(a) * int(b) for a, b in zip(t[i].tolist(), t[j].tolist())) for j in range(2)] for i in range(2)]
    assert g.tolist() == want and area2 == [sum(t[0].tolist()), sum(t[1].tolist())]
    assert 2 ** 63 <= min(min(r) for r in want) and max(max(r) for r in want) < 2 ** 64
    u = t.astype(np.uint64)
    assert [[int(v) for v in r] for r in u.dot(u.T)] == want
    with pytest.raises(ValueError, match="2\\^23"):
        ref.grams_exact(np.array([[2 ** 23]]), np.array([[1]]))


def test_the_module_refuses_before_any_device_work(scores, monkeypatch):
    from phamers_amd import _lib, compare

    def no_device(*a, **k):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(_lib, "get_context", no_device)
    bad = scores.copy()
    bad[1, 3] = np.nan
    for fn in (compare.delong, compare.bootstrap, compare.cells):
        with pytest.raises(ValueError, match="Input contains NaN or infinity."):
            fn(bad, P)
        bad[1, 3] = np.inf
        with pytest.raises(ValueError, match="Input contains NaN or infinity."):
            fn(bad, P)
        with pytest.raises(ValueError, match="cells <= 256"):
            fn(np.zeros((257, 10)), 5)
        with pytest.raises(ValueError, match="scores must be"):
            fn(scores[0], P)
        for n_pos in (0, P + N, P + N + 1, -1):
            with pytest.raises(ValueError, match="n_pos"):
                fn(scores, n_pos)
    for fn in (compare.delong, compare.cells):
        with pytest.raises(ValueError, match="two rows of each class"):
            fn(scores, 1)
        with pytest.raises(ValueError, match="two rows of each class"):
            fn(scores, P + N - 1)
    for fn in (compare.bootstrap, compare.cells):
        with pytest.raises(ValueError, match="at most %d rows" % _lib.COMPARE_BOOT_MAX_ROWS):
            fn(np.zeros((1, _lib.COMPARE_BOOT_MAX_ROWS + 1)), 5)
    with pytest.raises(ValueError, match="baseline"):
        compare.cells(scores, P, baseline=5)
    with pytest.raises(ValueError, match="level"):
        compare.cells(scores, P, level=1.0)


def test_the_binding_knows_the_new_entry_points_and_the_header_limits():
    import os
    import re

    from phamers_amd import _lib
    from tests.helpers import REPO
    for name in ("phk_compare_create", "phk_compare_destroy", "phk_compare_placements", "phk_compare_grams", "phk_compare_bootstrap"):
        assert name in _lib.SIGNATURES, name
    assert _lib.Compare._destroy == "phk_compare_destroy"
    text = open(os.path.join(REPO, "include", "phamers_hip.h")).read()
    assert int(re.search(r"#define PHK_COMPARE_MAX_CELLS (\d+)", text).group(1)) == _lib.COMPARE_MAX_CELLS == 256
    rows = int(re.search(r"#define PHK_COMPARE_BOOT_MAX_ROWS (\d+)", text).group(1))
    assert rows == _lib.COMPARE_BOOT_MAX_ROWS and rows >= 32768


def test_adaptors_order_the_cells_as_the_grids_do():
    from phamers_amd import compare

    class Sweep(object):
        k_neighbors, k_clusters = [1, 3], [4, 8, 9]
        knn_scores = np.array([[1.0, -1.0, 1.0], [-1.0, -1.0, 1.0]])
        kmeans_scores = np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]])

        def combo_scores(self, i, j):
            return self.knn_scores[i] + self.kmeans_scores[j]
    m = compare.combo_cells(Sweep())
    assert m.shape == (6, 3) and np.array_equal(m[4], Sweep.knn_scores[1] + Sweep.kmeans_scores[1])

    class Svm(object):
        classes_ = np.array([2, 7])
        held_decision = np.arange(2 * 2 * 5, dtype=np.float64).reshape(2, 2, 5)
    m, n_pos = compare.svm_cells(Svm(), [7, 2, 2, 7, 2])
    assert n_pos == 2 and m.shape == (4, 5) and m[3].tolist() == [15.0, 18.0, 16.0, 17.0, 19.0]

    L = {"pos_under_pos": np.array([[1.0, 2.0], [3.0, 4.0]]), "neg_under_pos": np.array([[5.0], [6.0]]),
         "pos_under_neg": np.array([[0.5, 0.25]]), "neg_under_neg": np.array([[0.125]])}
    m = compare.density_cells(L)
    assert m.tolist() == [[0.5, 1.75, 4.875], [2.5, 3.75, 5.875]]
