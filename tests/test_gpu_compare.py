"""The paired ROC-area comparison on the device (phamers_amd/compare.py, phk_compare_*) against the statement
tests/compare_ref.py: everything for equality -- the device sums are integers and every float is one rounding of an exact
rational -- except z (three roundings: 4 ulp) and p (1e-15 absolute)."""
import numpy as np
import pytest

from tests import compare_ref as ref
from tests import evaluate_ref

pytestmark = pytest.mark.gpu

CASES = evaluate_ref.cases()
SMALL = (37, 45)


def _stack(name):
    pos, neg = CASES[name]
    return np.concatenate((pos, neg))[None, :], len(pos)


def _groups(smallest_class=2):
    """the cases whose shapes agree, stacked as the cells of one call (DeLong needs two rows of each class)"""
    by_shape = {}
    for name, (pos, neg) in CASES.items():
        by_shape.setdefault((len(pos), len(neg)), []).append(name)
    return [names for (p, n), names in by_shape.items() if len(names) > 1 and min(p, n) >= smallest_class]


def _assert_delong_equals_statement(d, scores, n_pos):
    t_pos, t_neg = ref.placements(scores, n_pos)
    area2, g10, g01 = ref.grams(t_pos, t_neg)
    assert d.placements_positive.dtype == np.uint32 and np.array_equal(d.placements_positive, t_pos)
    assert d.placements_negative.dtype == np.uint32 and np.array_equal(d.placements_negative, t_neg)
    assert d.area2 == area2 and all(isinstance(a, int) for a in d.area2)
    assert d.gram_positive.dtype == np.uint64 and np.array_equal(d.gram_positive.astype(object), g10)
    assert np.array_equal(d.gram_negative.astype(object), g01)


# ---- 1. placements, area2 and both Grams on the evaluation cases --------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if min(len(CASES[n][0]), len(CASES[n][1])) >= 2])
def test_case_alone(name):
    from phamers_amd import compare, learning
    scores, n_pos = _stack(name)
    d = compare.delong(scores, n_pos)
    _assert_delong_equals_statement(d, scores, n_pos)
    labels = np.r_[np.ones(n_pos, np.uint8), np.zeros(scores.shape[1] - n_pos, np.uint8)]
    assert d.area2[0] == learning.roc_points(scores[0], labels)[3]
    assert d.auc[0] == evaluate_ref.rates(*(evaluate_ref.roc_points(scores[0], labels)[i] for i in (0, 1, 3)))[2]


@pytest.mark.parametrize("names", _groups(), ids="+".join)
def test_cases_stacked(names):
    from phamers_amd import compare
    scores, n_pos = np.vstack([_stack(n)[0] for n in names]), len(CASES[names[0]][0])
    _assert_delong_equals_statement(compare.delong(scores, n_pos), scores, n_pos)


def test_the_stacks_cover_a_pair_and_single_rows_stack_for_the_bootstrap():
    from phamers_amd import compare
    assert _groups() == [["separated", "inverted"]] and ["one_one", "two_tied"] in _groups(1)
    scores = np.vstack([_stack(n)[0] for n in ("one_one", "two_tied")])
    assert np.array_equal(compare.bootstrap(scores, 1, resamples=2, seed=1).area2, [[2, 1], [2, 1]])


@pytest.mark.parametrize("name", ["one_one", "two_tied", "one_many", "many_one"])
def test_a_class_of_one_row_is_refused_by_delong_and_runs_through_the_bootstrap(name):
    from phamers_amd import compare
    scores, n_pos = _stack(name)
    with pytest.raises(ValueError, match="two rows of each class"):
        compare.delong(scores, n_pos)
    with compare.Comparison(scores, n_pos) as c:
        with pytest.raises(ValueError, match="two rows of each class"):
            c.delong()
        got = c.bootstrap(3, seed=4)
    assert got.area2.dtype == np.uint64 and np.array_equal(got.area2, ref.bootstrap_brute(scores, n_pos, 4, 3))


# ---- 2. the Gram kernel's tiling ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, (700, 800)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("C", [1, 2, 32, 33, 65])   # one cell past one and past two pair tiles of 32
def test_gram_tiling_and_covariance(C, shape):
    from phamers_amd import compare
    P, N = shape
    scores = ref.noisy_cells(np.random.RandomState(100 + C), P, N, C)
    assert scores.shape == (C, P + N)
    d = compare.delong(scores, P)
    _assert_delong_equals_statement(d, scores, P)
    st = ref.Statement(scores, P)
    want = st.covariance()
    assert d.covariance.shape == (C, C) and np.array_equal(d.covariance, want)       # bit for bit
    assert np.array_equal(d.covariance, d.covariance.T)
    assert np.array_equal(d.auc, st.auc()) and np.array_equal(d.se, np.sqrt(np.diag(want)))
    if C >= 3:   # the last cell duplicates cell 0
        assert d.delta(0, C - 1) == 0.0 and d.delta_variance(0, C - 1) == 0.0
        assert np.isnan(d.z(0, C - 1)) and np.isnan(d.p_value(0, C - 1))
        pair = d.against(C - 1)
        assert pair["delta"][0] == 0.0 and np.isnan(pair["z"][0]) and np.isnan(pair["p"][0])
        assert pair["delta"][1] == st.delta(1, C - 1) and pair["delta_variance"][1] == st.delta_variance(1, C - 1)


# ---- 3. the bootstrap ----------------------------------------------------------------------------------------------------------
def _boot_cells(P, N, seed):
    return np.vstack((ref.noisy_cells(np.random.RandomState(seed), P, N, 4), np.full(P + N, 0.25)))   # ..., +-1, duplicate, all equal


@pytest.mark.parametrize("seed", [0, 2 ** 63 + 5])
@pytest.mark.parametrize("shape", [SMALL, (300, 212), (301, 212)], ids=lambda s: "%dx%d" % s)   # under / exactly two / past two chunks
def test_bootstrap_equals_brute_force(shape, seed):
    from phamers_amd import compare
    P, N = shape
    scores = _boot_cells(P, N, 7)
    want = ref.bootstrap_brute(scores, P, seed, 70)
    assert np.all(want[:, 4] == P * N)
    with compare.Comparison(scores, P) as c:
        for B in (1, 3, 70):
            for per_launch in (0, 16):   # 70 = 4 launches of 16 and one of 6
                got = c.bootstrap(B, seed=seed, _per_launch=per_launch)
                assert got.area2.shape == (B, 5) and np.array_equal(got.area2, want[:B]), (B, per_launch)
    assert np.array_equal(got.auc, ref.boot_auc(want, P, N))
    lo, hi = got.interval(0.9)
    qs = [(1.0 - 0.9) / 2.0, (1.0 + 0.9) / 2.0]      # the definition's expressions, not their decimal neighbours
    q = np.quantile(ref.boot_auc(want, P, N), qs, axis=0)
    assert np.array_equal(lo, q[0]) and np.array_equal(hi, q[1])
    assert got.delta_interval(0, 1, 0.9) == tuple(np.quantile(ref.boot_delta(want, 0, 1, P, N), qs))
    assert got.delta_interval(0, 3) == (0.0, 0.0)   # the duplicate sees the same resamples
    assert np.array_equal(compare.bootstrap(scores, P, resamples=3, seed=seed).area2, want[:3])


def test_bootstrap_at_the_row_limit_and_one_row_past_it():
    from phamers_amd import _lib, compare
    n = _lib.COMPARE_BOOT_MAX_ROWS
    P = 30000
    rng = np.random.RandomState(5)
    scores = np.vstack((np.round(np.r_[rng.normal(0.3, 1, P), rng.normal(0, 1, n + 1 - P)], 2), np.full(n + 1, 0.25)))
    got = compare.bootstrap(scores[:, :n], P, resamples=2, seed=9)
    assert np.array_equal(got.area2, ref.bootstrap_runs(scores[:, :n], P, 9, 2))
    with pytest.raises(ValueError, match="at most %d rows" % n):
        compare.bootstrap(scores, P, resamples=2, seed=9)
    h = _lib.Compare(_lib.get_context(), scores, P)          # the library's own refusal
    try:
        with pytest.raises(ValueError, match="at most %d rows" % n):
            h.bootstrap(9, 2)
    finally:
        h.close()


# ---- 4. repeat calls and call order --------------------------------------------------------------------------------------------
def test_repeat_calls_in_either_order_and_closing_twice():
    from phamers_amd import compare
    P, N = SMALL
    scores = _boot_cells(P, N, 8)

    def same(d, e):
        return d.area2 == e.area2 and np.array_equal(d.covariance, e.covariance) and \
            np.array_equal(d.placements_positive, e.placements_positive) and \
            np.array_equal(d.placements_negative, e.placements_negative) and \
            np.array_equal(d.gram_positive, e.gram_positive) and np.array_equal(d.gram_negative, e.gram_negative)
    a = compare.Comparison(scores, P)
    d1, b1, d2, b2 = a.delong(), a.bootstrap(20, seed=3), a.delong(), a.bootstrap(20, seed=3)
    a.close()
    a.close()
    with pytest.raises(ValueError, match="closed"):
        a.delong()
    b = compare.Comparison(scores, P)
    b3, d3, b4, d4 = b.bootstrap(20, seed=3), b.delong(), b.bootstrap(20, seed=3), b.delong()
    b.close()
    b.close()
    assert same(d1, d2) and same(d1, d3) and same(d1, d4)
    for other in (b2, b3, b4):
        assert np.array_equal(b1.area2, other.area2)
    assert np.array_equal(b1.area2, ref.bootstrap_brute(scores, P, 3, 20))
    assert not np.array_equal(b1.area2, compare.bootstrap(scores, P, 20, seed=4).area2)


def test_the_library_refuses_what_the_header_says():
    from phamers_amd import _lib
    ctx = _lib.get_context()
    for scores, n_pos in ((np.zeros((0, 4)), 2), (np.zeros((257, 4)), 2), (np.zeros((1, 4)), 0), (np.zeros((1, 4)), 4)):
        with pytest.raises(ValueError):
            _lib.Compare(ctx, scores, n_pos)
    with pytest.raises(ValueError, match="Input contains NaN or infinity."):
        _lib.Compare(ctx, np.array([[0.0, np.inf, 1.0, 2.0]]), 2)


# ---- 5. end to end: the combo grid's cells, the table and the command line ---------------------------------------------------------
def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_combo_cells_table_and_command_line(tmp_path):
    from phamers_amd import combo_grid, compare, fileIO, kmer
    from tests import helpers
    counts = helpers.load_npz("ref_features.npz")
    files = []
    for tag, rows in (("pos", 300), ("neg", 320)):
        path = tmp_path / (tag + "_features.csv")
        with open(path, "w") as f:
            for i, row in enumerate(counts[tag + "_counts"][:rows].astype(np.int64)):
                f.write("%s_%d,%s\n" % (tag, i, ",".join("%d" % c for c in row)))
        files.append(str(path))
    pos, neg = (kmer.normalize_counts(fileIO.read_feature_file(p)[1]) for p in files)
    sweep = combo_grid.sweep(pos, neg, [1, 3], [4, 8], 3, seed=0)
    m = compare.combo_cells(sweep)
    assert m.shape == (4, 620)
    table = compare.cells(m, 300, resamples=300)
    assert np.array_equal(table["auc"], sweep.combo_auc.ravel())
    want = ref.cells(m, 300, baseline=0, resamples=300, seed=0, level=0.95)
    assert np.array_equal(table["auc"], want["auc"])
    assert np.array_equal(table["se"] ** 2, want["se"] ** 2) and np.array_equal(table["se"], np.sqrt(want["variance"]))
    assert np.array_equal(table["delta"], want["delta"])
    assert np.array_equal(table["delta_se"], np.sqrt(want["delta_variance"]))
    for name in ("ci_low", "ci_high", "boot_low", "boot_high", "boot_delta_low", "boot_delta_high"):
        assert np.array_equal(table[name], want[name]), name
    assert table["delta"][0] == 0.0 and np.isnan(table["z"][0]) and np.isnan(table["p"][0])
    assert np.all(_ulps(table["z"][1:], want["z"][1:]) <= 4)
    assert np.all(np.abs(table["p"][1:] - want["p"][1:]) <= 1e-15)
    assert np.all(table["boot_low"] <= table["auc"]) and np.all(table["auc"] <= table["boot_high"])

    out = str(tmp_path / "compare.csv")
    argv = ["-pf", files[0], "-nf", files[1], "--k_neighbors", "1", "3", "--k_clusters", "4", "8", "-N", "3", "--seed", "0",
            "--resamples", "300", "-out", out]
    assert compare.main(argv) == 0
    assert open(out).readline().startswith("# ")
    back = np.loadtxt(out, delimiter=",", comments="#")
    assert back.shape == (4, 2 + len(compare.COLUMNS))
    assert back[:, 0].tolist() == [1, 1, 3, 3] and back[:, 1].tolist() == [4, 8, 4, 8]
    for k, name in enumerate(compare.COLUMNS):
        assert np.array_equal(back[:, 2 + k], table[name], equal_nan=True), name
    assert compare.main(argv[:-2] + ["--baseline", "3", "8", "-out", out]) == 0
    again = compare.cells(m, 300, baseline=3, resamples=300)
    back = np.loadtxt(out, delimiter=",", comments="#")
    for k, name in enumerate(compare.COLUMNS):
        assert np.array_equal(back[:, 2 + k], again[name], equal_nan=True), name
    text = [line for line in open(out) if not line.startswith("#")][1].split(",")
    assert text[2] == repr(float(again["auc"][1]))   # the notation of the other grids' tables
