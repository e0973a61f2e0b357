"""GPU: combo_grid.hip past the shapes of tests/test_gpu_combo_grid.py, against the NumPy statement (tests/combo_grid_ref.py)
and not against the single-cell path, which runs the same device code.  Sections 1-4 drive the resident object
(``_lib.ComboGrid``) with fold ids and centroids of the test's own, so that no FoldPlan and no k-means stand between the
input and the kernel under test; section 5 goes through ``combo_grid.sweep`` for the fold row source.

  1. the neighbour word to bit 63 (k_neighbors up to 64, the even split at 64);
  2. the pair pass at the tile edges of M and the column-step edges of D, with a fold that holds nothing and one of a
     single row, in one launch and in launches of 64 query rows;
  3. the centroid pass in steps of one query tile, with segments of 1, 63, 64, 65 and 130 columns;
  4. both halves in one call;
  5. the fold k-means at D = 2, 63, 65 and 257 with classes of 70 and 31 rows.

The votes are bits; the k-means half is held to the bar of test_seventy_folds_against_the_numpy_statement, 4 eps relative
to the statement's value: the chains are the statement's bit for bit, so are their square roots and the quotient, and the
two tanh implementations are each within an ulp or two of the true value."""
import numpy as np
import pytest

from tests import combo_grid_ref as ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Grid(object):
    """A resident grid on rows, fold ids and classes of the test's own."""

    def __init__(self, X, fold_of, is_pos, F):
        from phamers_amd import _lib
        self.F, self.D = F, X.shape[1]
        self.cg = _lib.ComboGrid(_lib.get_context(), X, fold_of, is_pos, F)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.cg.close()

    def bank(self, ku, rows):
        """An empty bank for the values ``ku`` (a fit without problems allocates and zeroes it), filled with ``rows``."""
        n = self.F * 2 * sum(ku)
        assert rows.shape == (n, self.D)
        self.cg.fit([], [], [], [], np.zeros((2 * self.F, self.D)), np.zeros(2 * self.F), n, [])
        assert not self.cg.get_centroids(0, n).any()
        self.cg.put_centroids(0, rows)
        assert same_bits(self.cg.get_centroids(0, n), rows)

    def score(self, kn, ku, rows_per_pass=0):
        return self.cg.score(list(kn), list(ku), rows_per_pass=rows_per_pass)


def centroids_of(bank, ku, F, j):
    """{fold: (positive, negative)} of value j in a bank laid out as the header says."""
    Ksum, koff = sum(ku), np.concatenate(([0], np.cumsum(ku)))
    out = {}
    for f in range(F):
        at = f * 2 * Ksum
        out[f] = (bank[at + koff[j]:at + koff[j + 1]], bank[at + Ksum + koff[j]:at + Ksum + koff[j + 1]])
    return out


# ---- 1. the neighbour word to its full width ---------------------------------------------------------------------------
def test_the_neighbour_word_is_read_to_bit_63():
    """k_neighbors = 1, 2, 31, 32, 33, 63, 64 in one call.  A word built or masked with a 32-bit shift cannot pass: it
    leaves bits 32-63 zero, so at k = 64 a row counts at most its first 32 neighbours, and the conditions asserted of the
    statement below -- rows whose 64th neighbour is positive, rows whose vote at 64 differs from that at 63, rows split
    32 : 32 -- name rows where those bits decide (a shift count taken modulo 32 instead moves bit 63 to bit 31 and fails
    at k = 31, 32 and 33)."""
    X, fold_of, is_pos = ref.word_fixture()
    ks = (1, 2, 31, 32, 33, 63, 64)
    nb = ref.neighbour_bits(X, fold_of, is_pos, 64)
    want = {k: ref.votes(nb, k) for k in ks}
    assert (nb.sum(axis=1) == 32).any() and (want[64][nb.sum(axis=1) == 32] == -1.0).all()
    assert (want[63] != want[64]).any()
    assert nb[:, 63].any() and not nb[:, 63].all()
    for k in ks:
        assert (want[k] == 1.0).any() and (want[k] == -1.0).any(), k
    with Grid(X, fold_of, is_pos, 3) as g:
        for call in (ks, (64, 63, 33, 33, 32, 31, 2, 1), (64,)):
            knn, km = g.score(call, ())
            assert knn.shape == (len(call), 200) and km.shape == (0, 200)
            for i, k in enumerate(call):
                assert np.array_equal(knn[i], want[k]), (call, k, np.flatnonzero(knn[i] != want[k]))
        with pytest.raises(ValueError, match="k_neighbors"):
            g.score((65,), ())


# ---- 2. tile and column-step edges of the pair pass ----------------------------------------------------------------------
KN_EDGE = (1, 2, 5)


def _assert_votes(X, fold_of, is_pos, what):
    nb = ref.neighbour_bits(X, fold_of, is_pos, max(KN_EDGE))
    with Grid(X, fold_of, is_pos, 4) as g:
        one, _ = g.score(KN_EDGE, ())
        split, _ = g.score(KN_EDGE, (), rows_per_pass=64)
    for i, k in enumerate(KN_EDGE):
        want = ref.votes(nb, k)
        assert np.array_equal(one[i], want), (what, k, np.flatnonzero(one[i] != want))
    assert same_bits(one, split), what
    return nb


@pytest.mark.parametrize("D", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("M", [63, 64, 65, 127, 128, 129])
def test_votes_at_the_tile_edges(M, D):
    rng = np.random.RandomState(100 * M + D)
    is_pos = rng.rand(M) < 0.5
    X = rng.randn(M, D) + 0.5 * is_pos[:, None]
    fold_of = ref.edge_folds(M)
    held = np.bincount(fold_of, minlength=4)
    assert held[2] == 0 and held[3] == 1 and held[0] != held[1]
    nb = _assert_votes(X, fold_of, is_pos, (M, D))
    assert nb.any() and not nb.all()


@pytest.mark.parametrize("M", [63, 64, 65, 127, 128, 129])
def test_votes_of_tied_rows_at_the_tile_edges(M):
    """Integer-valued rows: exact distance ties and duplicates across the classes and the folds decide the order."""
    X, is_pos = ref.tie_rows(M)
    fold_of = ref.edge_folds(M)
    same = (X[:, None, :] == X[None, :, :]).all(axis=2) & ~np.eye(M, dtype=bool)
    other_fold = fold_of[:, None] != fold_of[None, :]
    assert (same & other_fold & (is_pos[:, None] != is_pos[None, :])).any() and (same & ~other_fold).any()
    _assert_votes(X, fold_of, is_pos, M)


# ---- 3. the centroid pass with centroids of the test's own -----------------------------------------------------------
KU = (1, 63, 64, 65, 130)


def _planted(seed, M, D, fold_of, ku, F):
    """Random rows and a random bank, with one held-out row of fold 0 as the last positive centroid of every segment of
    its fold and one of fold 1 as the last negative centroid: (X, bank, planted positive row, planted negative row)."""
    rng = np.random.RandomState(seed)
    X = rng.randn(M, D)
    Ksum, koff = sum(ku), np.concatenate(([0], np.cumsum(ku)))
    bank = rng.randn(F * 2 * Ksum, D)
    a, b = np.flatnonzero(fold_of == 0)[-1], np.flatnonzero(fold_of == 1)[-1]
    for j in range(len(ku)):
        bank[0 * 2 * Ksum + koff[j + 1] - 1] = X[a]
        bank[1 * 2 * Ksum + Ksum + koff[j + 1] - 1] = X[b]
    return X, bank, a, b


def _assert_kmeans_half(got, X, fold_of, bank, ku, F, what):
    worst = 0.0
    for j in range(len(ku)):
        want = ref.kmeans_scores_for(X, fold_of, centroids_of(bank, ku, F, j))
        assert not np.isnan(want).any()
        err = np.abs(got[j] - want)
        worst = max(worst, float(np.max(err / np.abs(want))))
        assert np.all(err <= 4 * EPS * np.abs(want)), (what, ku[j], np.flatnonzero(err > 4 * EPS * np.abs(want)))
    print("%s: k-means half, largest deviation %.3e relative (allowed %.3e): %.2f of the bar" % (what, worst, 4 * EPS, worst / (4 * EPS)))


@pytest.fixture(scope="module")
def three_tiles():
    """M = 300, D = 33, two folds of 150 rows each: three query tiles per fold; the bank of KU.  Scored with
    rows_per_pass = 0, 64 (three launches of the centroid pass, xtile0 = 0, 1, 2) and 128."""
    M, D, F = 300, 33, 2
    fold_of = np.arange(M) % 2
    is_pos = np.arange(M) % 3 == 0
    X, bank, a, b = _planted(21, M, D, fold_of, KU, F)
    got = {}
    with Grid(X, fold_of, is_pos, F) as g:
        g.bank(KU, bank)
        for rpp in (0, 64, 128):
            got[rpp] = g.score((), KU, rows_per_pass=rpp)
        both = g.score((3, 64), KU, rows_per_pass=64)
        knn_only = g.score((3, 64), ())
    return X, fold_of, is_pos, bank, a, b, got, both, knn_only


def test_centroid_pass_in_steps_of_query_tiles(three_tiles):
    X, fold_of, is_pos, bank, a, b, got, _, _ = three_tiles
    for rpp in (0, 64, 128):
        knn, km = got[rpp]
        assert knn.shape == (0, 300) and km.shape == (len(KU), 300)
        assert same_bits(km, got[0][1]), rpp
        _assert_kmeans_half(km, X, fold_of, bank, KU, 2, "rows_per_pass=%d" % rpp)
    km = got[64][1]
    for j in range(len(KU)):       # ep = 0: (en - 0) / (0 + en) = 1 exactly; en = 0: -1
        assert abs(km[j, a] - np.tanh(1.0)) <= 4 * EPS * np.tanh(1.0), (KU[j], km[j, a])
        assert abs(km[j, b] - np.tanh(-1.0)) <= 4 * EPS * np.tanh(1.0), (KU[j], km[j, b])


def test_centroid_pass_with_a_short_fold_and_a_fold_without_rows():
    """Held-out sets of 130, 3, 0 and 67 rows against one segment of 65 columns: query tiles past a short fold's end,
    a fold whose blocks all return at once."""
    M, D, F, ku = 200, 33, 4, (65,)
    fold_of = np.r_[np.zeros(130, int), np.ones(3, int), np.full(67, 3)]
    fold_of = fold_of[np.random.RandomState(22).permutation(M)]
    assert np.bincount(fold_of, minlength=4).tolist() == [130, 3, 0, 67]
    is_pos = np.arange(M) % 2 == 0
    X, bank, a, b = _planted(23, M, D, fold_of, ku, F)
    with Grid(X, fold_of, is_pos, F) as g:
        g.bank(ku, bank)
        _, km = g.score((), ku)
        _, split = g.score((), ku, rows_per_pass=64)
    assert same_bits(km, split)
    _assert_kmeans_half(km, X, fold_of, bank, ku, F, "folds of 130, 3, 0, 67")
    assert abs(km[0, a] - np.tanh(1.0)) <= 4 * EPS * np.tanh(1.0) and abs(km[0, b] - np.tanh(-1.0)) <= 4 * EPS * np.tanh(1.0)


# ---- 4. both halves in one call ---------------------------------------------------------------------------------------
def test_both_halves_in_one_call_equal_each_half_alone(three_tiles):
    X, fold_of, is_pos, bank, a, b, got, both, knn_only = three_tiles
    assert same_bits(both[0], knn_only[0]) and knn_only[1].shape == (0, 300)
    assert same_bits(both[1], got[0][1])
    nb = ref.neighbour_bits(X, fold_of, is_pos, 64)
    for i, k in enumerate((3, 64)):
        assert np.array_equal(both[0][i], ref.votes(nb, k)), k


# ---- 5. the fold row source at other widths and unequal classes -----------------------------------------------------------
KC5 = (1, 2, 5)


@pytest.mark.parametrize("D", [2, 63, 65, 257])
def test_fold_k_means_at_other_widths_with_unequal_classes(D):
    """Classes of 70 and 31 rows in three folds: train sets of 46 or 47 and of 20 or 21 rows, so the chunks are cut at
    four sizes; D = 65 is a partial second trip of the 64-lane column loops, D = 257 a second trip of the 256-thread ones."""
    from phamers_amd import combo_grid, learning
    P, N = ref.blob_rows(31, 70, D), ref.blob_rows(32, 31, D)
    res = combo_grid.sweep(P, N, (3,), KC5, 3, seed=0)
    print("D = %d routes:" % D, list(zip(res.problems, res.routes)))
    assert len(res.routes) == 18
    assert 4 * res.routes.count("device") >= 3 * len(res.routes), list(zip(res.problems, res.routes))
    for (fold, cls, j), got in res.centroids.items():
        data, held = (P, res.plan.positive == fold) if cls == combo_grid.POSITIVE else (N, res.plan.negative == fold)
        train = data[~held]
        want = learning.get_centroids(train, learning.kmeans(train, KC5[j]))
        assert same_bits(got, want), (D, fold, cls, KC5[j], res.routes[res.problems.index((fold, cls, KC5[j]))])
    X = np.vstack((P, N))
    fold_of = np.concatenate((res.plan.positive, res.plan.negative))
    worst = 0.0
    for j in range(len(KC5)):
        cents = {f: (res.centroids[(f, combo_grid.POSITIVE, j)], res.centroids[(f, combo_grid.NEGATIVE, j)]) for f in range(3)}
        want = ref.kmeans_scores(P, N, 3, 0, cents)
        assert same_bits(want, ref.kmeans_scores_for(X, fold_of, cents))
        err = np.abs(res.kmeans_scores[j] - want)
        worst = max(worst, float(np.max(err / np.abs(want))))
        assert np.all(err <= 4 * EPS * np.abs(want)), (D, KC5[j])
    print("D = %d: k-means half, largest deviation %.3e relative (allowed %.3e): %.2f of the bar" % (D, worst, 4 * EPS, worst / (4 * EPS)))
    is_pos = np.r_[np.ones(70, bool), np.zeros(31, bool)]
    assert np.array_equal(res.knn_scores[0], ref.votes(ref.neighbour_bits(X, fold_of, is_pos, 3), 3))
    for chunk in (1, 2):
        other = combo_grid.sweep(P, N, (3,), KC5, 3, seed=0, _chunk=chunk)
        assert other.routes == res.routes
        assert same_bits(other.knn_scores, res.knn_scores) and same_bits(other.kmeans_scores, res.kmeans_scores)
        assert same_bits(other.combo_auc, res.combo_auc) and same_bits(other.kmeans_auc, res.kmeans_auc)
        for key, c in res.centroids.items():
            assert same_bits(other.centroids[key], c), (chunk, key)
