"""GPU: the k_neighbors x k_clusters grid (combo_grid.hip, phamers_amd.combo_grid) against what it batches -- one
``cross_validator`` run per cell -- bit for bit on the exact route, against the NumPy statement of a cell
(tests/combo_grid_ref.py) where the validator cannot say (ties, folds past 63), and against itself for everything a cell
must not depend on."""
import numpy as np
import pytest

from tests import combo_grid_ref as ref
from tests import neighbors_ref

pytestmark = pytest.mark.gpu

FOLDS, SEED = 3, 0
KN, KC = (1, 2, 3, 4, 8), (2, 5)
EPS = np.finfo(np.float64).eps


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


_fits = {}


def _validator():
    """A cross_validator whose per-fold fit -- get_centroids(train, learning.kmeans(train, k)), its default -- is computed
    once per (train rows, k) for the whole module: the methods kmeans and combo ask for the same fits."""
    from phamers_amd import cross_validate, learning

    class Validator(cross_validate.cross_validator):
        def _fold_centroids(self, train_rows):
            assert self.kmeans == 'sklearn'
            key = (train_rows.shape, hash(train_rows.tobytes()), self.k_clusters)
            if key not in _fits:
                _fits[key] = learning.get_centroids(train_rows, learning.kmeans(train_rows, self.k_clusters))
            return _fits[key]
    return Validator()


def validate(P, N, method, folds, seed, k_neighbors=3, k_clusters=86, exact=True):
    """(scores in vstack order, auc, accuracy) of one validator run."""
    from phamers_amd import _lib, learning
    v = _validator()
    v.positive_data, v.negative_data, v.method, v.N, v.seed = P, N, method, folds, seed
    v.k_neighbors, v.k_clusters = k_neighbors, k_clusters
    ctx = _lib.get_context()
    if exact:
        with ctx.options(force_exact=("1", "0")):
            ps, ns = v.cross_validate()
    else:
        ps, ns = v.cross_validate()
    tp, fp, fn, tn = learning.truth_counts(ps, ns, threshold=0)
    return np.concatenate((ps, ns)), v.performance()[2], float(tp + tn) / (tp + fp + fn + tn)


@pytest.fixture(scope="module")
def blobs():
    return ref.blob_fixture()


@pytest.fixture(scope="module")
def base(blobs):
    from phamers_amd import combo_grid
    details = {}
    res = combo_grid.sweep(blobs[0], blobs[1], KN, KC, FOLDS, seed=SEED, _details=details)
    res.details = details
    return res


# ---- 1. cells ------------------------------------------------------------------------------------------------------------
def test_every_k_means_problem_of_the_fixture_ran_on_the_device(base):
    """Otherwise the tests below show nothing about the fold row source."""
    assert len(base.routes) == 2 * FOLDS * len(KC)
    assert base.routes == ["device"] * len(base.routes), list(zip(base.problems, base.routes))
    print("smallest seeding margin %.3e, smallest gap %.3e" % (base.details["seed_margin"].min(), base.details["min_gap"].min()))


def test_cells_equal_the_validator_bit_for_bit(base, blobs):
    P, N = blobs
    assert base.knn_scores.shape == (len(KN), 145) and base.kmeans_scores.shape == (len(KC), 145)
    assert base.combo_auc.shape == base.combo_accuracy.shape == (len(KN), len(KC))
    assert set(np.unique(base.knn_scores)) <= {-1.0, 1.0}
    for i, kn in enumerate(KN):
        s, auc, acc = validate(P, N, "knn", FOLDS, SEED, k_neighbors=kn)
        assert same_bits(base.knn_scores[i], s), kn
        assert base.knn_auc[i] == auc and base.knn_accuracy[i] == acc, kn
    for j, kc in enumerate(KC):
        s, auc, acc = validate(P, N, "kmeans", FOLDS, SEED, k_clusters=kc)
        assert same_bits(base.kmeans_scores[j], s), kc
        assert base.kmeans_auc[j] == auc and base.kmeans_accuracy[j] == acc, kc
    for i, kn in enumerate(KN):
        for j, kc in enumerate(KC):
            s, auc, acc = validate(P, N, "combo", FOLDS, SEED, k_neighbors=kn, k_clusters=kc)
            assert same_bits(base.combo_scores(i, j), s), (kn, kc)
            assert base.combo_auc[i, j] == auc and base.combo_accuracy[i, j] == acc, (kn, kc)


# ---- 2. centroids --------------------------------------------------------------------------------------------------------
def test_centroids_equal_numpy_s_means_of_the_reference_fit(base, blobs):
    from phamers_amd import combo_grid, learning
    P, N = blobs
    assert len(base.centroids) == 2 * FOLDS * len(KC)
    for (fold, cls, j), got in base.centroids.items():
        data, held = (P, base.plan.positive == fold) if cls == combo_grid.POSITIVE else (N, base.plan.negative == fold)
        train = data[~held]
        want = learning.get_centroids(train, learning.kmeans(train, KC[j]))
        assert same_bits(got, want), (fold, cls, KC[j])


# ---- 3. ties -------------------------------------------------------------------------------------------------------------
def test_tied_distances_are_ordered_by_index_with_the_own_fold_left_out():
    from phamers_amd import combo_grid
    P, N = ref.tie_fixture()
    ks = (1, 2, 3, 6)
    res = combo_grid.sweep(P, N, ks, (), 4, seed=SEED)
    assert res.kmeans_scores.shape == (0, 80) and res.routes == [] and res.combo_auc.shape == (4, 0)
    want = ref.knn_scores(P, N, 4, SEED, ks)
    for i, k in enumerate(ks):
        assert same_bits(res.knn_scores[i], want[i]), k
    assert (want[1] == -1.0).any() and (want[1] == 1.0).any()


# ---- 4. independence ---------------------------------------------------------------------------------------------------
def _assert_same_cells(a, ia, ja, b, ib, jb):
    for x, y in zip(ia, ib):
        assert same_bits(a.knn_scores[x], b.knn_scores[y]) and a.knn_auc[x] == b.knn_auc[y] and a.knn_accuracy[x] == b.knn_accuracy[y]
    for x, y in zip(ja, jb):
        assert same_bits(a.kmeans_scores[x], b.kmeans_scores[y]) and a.kmeans_auc[x] == b.kmeans_auc[y]
        for fold in range(FOLDS):
            for cls in (0, 1):
                assert same_bits(a.centroids[(fold, cls, x)], b.centroids[(fold, cls, y)])
    for x, y in zip(ia, ib):
        for u, w in zip(ja, jb):
            assert a.combo_auc[x, u] == b.combo_auc[y, w] and a.combo_accuracy[x, u] == b.combo_accuracy[y, w]


@pytest.mark.parametrize("how", ["chunk", "rows_per_pass", "reversed", "alone"])
def test_a_cell_does_not_depend_on_the_rest_of_the_call(base, blobs, how):
    from phamers_amd import combo_grid
    P, N = blobs
    all_i, all_j = range(len(KN)), range(len(KC))
    if how == "chunk":
        other = combo_grid.sweep(P, N, KN, KC, FOLDS, seed=SEED, _chunk=1)
        _assert_same_cells(base, all_i, all_j, other, all_i, all_j)
    elif how == "rows_per_pass":
        other = combo_grid.sweep(P, N, KN, KC, FOLDS, seed=SEED, _rows_per_pass=64)
        _assert_same_cells(base, all_i, all_j, other, all_i, all_j)
    elif how == "reversed":
        kn, kc = (8, 4, 3, 3, 2, 1), (5, 2, 5)
        other = combo_grid.sweep(P, N, kn, kc, FOLDS, seed=SEED)
        assert other.k_neighbors == list(kn) and other.k_clusters == list(kc)
        assert other.knn_scores.shape[0] == 6 and other.kmeans_scores.shape[0] == 3 and other.combo_auc.shape == (6, 3)
        _assert_same_cells(base, [KN.index(k) for k in kn], [KC.index(k) for k in kc], other, range(6), range(3))
    else:
        other = combo_grid.sweep(P, N, (), (5,), FOLDS, seed=SEED)
        assert other.knn_scores.shape == (0, 145)
        _assert_same_cells(base, [], [1], other, [], [0])
    assert other.routes == ["device"] * len(other.routes)


# ---- 5. many folds -------------------------------------------------------------------------------------------------------
def test_seventy_folds_against_the_numpy_statement(blobs):
    """Held-out sets of one or two rows, fold ids past 63."""
    from phamers_amd import combo_grid
    P, N = blobs
    kn = (1, 3)
    res = combo_grid.sweep(P, N, kn, (3,), 70, seed=SEED)
    assert res.plan.positive.max() == 69 and len(res.routes) == 140
    want = ref.knn_scores(P, N, 70, SEED, kn)
    for i, k in enumerate(kn):
        assert same_bits(res.knn_scores[i], want[i]), k
    cents = {f: (res.centroids[(f, combo_grid.POSITIVE, 0)], res.centroids[(f, combo_grid.NEGATIVE, 0)]) for f in range(70)}
    km = ref.kmeans_scores(P, N, 70, SEED, cents)
    err = np.abs(res.kmeans_scores[0] - km)
    print("k-means half: largest deviation %.3e relative (allowed %.3e)" % (np.max(err / np.abs(km)), 4 * EPS))
    assert np.all(err <= 4 * EPS * np.abs(km))
    host = res.routes.count("host")
    print("%d of %d k-means problems went through the host" % (host, len(res.routes)))
    assert 4 * host <= len(res.routes), "the fixture is wrong for this test: %d of %d problems were declined by the device" % (
        host, len(res.routes))


# ---- 6. the reference rows ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference(golden_dir):
    from phamers_amd import combo_grid
    X, _, n_pos = neighbors_ref.reference_rows(golden_dir)
    P, N = np.ascontiguousarray(X[:n_pos]), np.ascontiguousarray(X[n_pos:])
    assert (len(P), len(N), X.shape[1]) == (2255, 2418, 256)
    return P, N, combo_grid.sweep(P, N, (3, 5), (86,), 4, seed=SEED)


def test_reference_rows_equal_the_validator_on_the_exact_route(reference):
    P, N, res = reference
    print("routes:", res.routes)
    for i, kn in enumerate((3, 5)):
        s, auc, acc = validate(P, N, "knn", 4, SEED, k_neighbors=kn)
        assert same_bits(res.knn_scores[i], s), kn
        assert res.knn_auc[i] == auc and res.knn_accuracy[i] == acc
    s, auc, acc = validate(P, N, "kmeans", 4, SEED, k_clusters=86)
    assert same_bits(res.kmeans_scores[0], s)
    assert res.kmeans_auc[0] == auc and res.kmeans_accuracy[0] == acc
    for i, kn in enumerate((3, 5)):
        s, auc, acc = validate(P, N, "combo", 4, SEED, k_neighbors=kn, k_clusters=86)
        assert same_bits(res.combo_scores(i, 0), s), kn
        assert res.combo_auc[i, 0] == auc and res.combo_accuracy[i, 0] == acc


def test_reference_rows_agree_with_the_validator_s_default_route(reference):
    """There the final distances are summed in another order (exact_d2): equal votes, and the k-means half within
    4 D 2^-53 absolute -- each chain of D non-negative terms within D 2^-53 relative on either route, halved by the square
    root, the argument of tanh moved by at most that much per route, tanh of slope <= 1."""
    P, N, res = reference
    s, _, _ = validate(P, N, "knn", 4, SEED, k_neighbors=3, exact=False)
    assert same_bits(res.knn_scores[0], s)
    s, _, _ = validate(P, N, "kmeans", 4, SEED, k_clusters=86, exact=False)
    err = np.abs(res.kmeans_scores[0] - s)
    print("k-means half: largest deviation %.3e (allowed %.3e)" % (err.max(), 4 * 256 * 2.0 ** -53))
    assert np.all(err <= 4 * 256 * 2.0 ** -53)


# ---- 7. errors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["nan", "k_neighbors", "k_clusters", "empty"])
def test_an_error_leaves_the_context_usable(base, blobs, case):
    from phamers_amd import combo_grid
    P, N = blobs
    with pytest.raises(ValueError):
        if case == "nan":
            bad = N.copy()
            bad[7, 3] = np.nan
            combo_grid.sweep(P, bad, (3,), (5,), FOLDS, seed=SEED)
        elif case == "k_neighbors":
            combo_grid.sweep(P, N, (3, 97), (5,), FOLDS, seed=SEED)    # train sets: 96, 97, 97 rows -- the smallest is 96
        elif case == "k_clusters":
            combo_grid.sweep(P, N, (3,), (5, 47), FOLDS, seed=SEED)    # the positive class's train sets: 46, 47, 47
        else:
            combo_grid.sweep(P, N, (), (), FOLDS, seed=SEED)
    again = combo_grid.sweep(P, N, (3,), (5,), FOLDS, seed=SEED)
    assert same_bits(again.knn_scores[0], base.knn_scores[2]) and same_bits(again.kmeans_scores[0], base.kmeans_scores[1])


def test_device_refuses_what_the_module_checks(blobs):
    """The C entry points make the same checks of their own (PHK_ERR_ARG -> ValueError), and a refused call leaves the
    handle usable."""
    from phamers_amd import _lib
    P, N = blobs
    X = np.vstack((P, N))
    fold_of = ref.fold_ids(70, 75, FOLDS, SEED)
    is_pos = np.r_[np.ones(70, np.uint8), np.zeros(75, np.uint8)]
    ctx = _lib.get_context()
    with pytest.raises(ValueError):
        _lib.ComboGrid(ctx, X, fold_of, is_pos, 1)
    with pytest.raises(ValueError):
        _lib.ComboGrid(ctx, X, fold_of + 1, is_pos, FOLDS)
    cg = _lib.ComboGrid(ctx, X, fold_of, is_pos, FOLDS)
    try:
        for kn in ([0], [65], [97]):
            with pytest.raises(ValueError, match="k_neighbors"):
                cg.score(kn, [])
        with pytest.raises(ValueError, match="bank"):
            cg.score([], [5])                                           # no bank yet
        with pytest.raises(ValueError):
            cg.score([], [])
        knn, _ = cg.score([3], [])
        assert same_bits(knn[0], ref.knn_scores(P, N, FOLDS, SEED, (3,))[0])
    finally:
        cg.close()


# ---- 8. the host route, the table and the command line -------------------------------------------------------------------
def test_sklearn_mode_sends_every_problem_through_the_host_with_the_same_bits(base, blobs, monkeypatch):
    from phamers_amd import combo_grid
    monkeypatch.setenv("PHAMERS_KMEANS", "sklearn")
    other = combo_grid.sweep(blobs[0], blobs[1], (3,), KC, FOLDS, seed=SEED)
    assert other.routes == ["host"] * (2 * FOLDS * len(KC)) and other.problems == base.problems
    _assert_same_cells(base, [2], range(len(KC)), other, [0], range(len(KC)))


def test_table_and_command_line(tmp_path):
    from phamers_amd import combo_grid, fileIO, kmer, transform_kmers
    from tests import helpers
    ref_counts = helpers.load_npz("ref_features.npz")
    files = []
    for tag in ("pos", "neg"):
        counts = ref_counts[tag + "_counts"][:150].astype(np.int64)
        path = tmp_path / (tag + "_features.csv")
        with open(path, "w") as f:
            for i, row in enumerate(counts):
                f.write("%s_%d,%s\n" % (tag, i, ",".join("%d" % c for c in row)))
        files.append(str(path))
    out = str(tmp_path / "grid.csv")
    argv = ["-pf", files[0], "-nf", files[1], "--k_neighbors", "1", "3", "--k_clusters", "4", "9", "4", "-N", "3", "--seed", "1", "-out", out]
    assert combo_grid.main(argv) == 0
    pos, neg = fileIO.read_feature_file(files[0], normalize=True)[1], fileIO.read_feature_file(files[1], normalize=True)[1]
    table = combo_grid.grid(pos, neg, [1, 3], [4, 9, 4], folds=3, seed=1)
    res = combo_grid.sweep(pos, neg, [1, 3], [4, 9, 4], 3, seed=1)
    assert table["k_neighbors"].tolist() == [1, 1, 1, 3, 3, 3] and table["k_clusters"].tolist() == [4, 9, 4, 4, 9, 4]
    assert np.array_equal(table["auc"], res.combo_auc.ravel()) and np.array_equal(table["accuracy"], res.combo_accuracy.ravel())
    assert np.array_equal(table["knn_auc"], np.repeat(res.knn_auc, 3)) and np.array_equal(table["kmeans_auc"], np.tile(res.kmeans_auc, 2))
    assert table["best"] == int(np.argmax(table["auc"])) and table["auc"][0] == table["auc"][2]
    back = combo_grid.read_grid(out)
    assert open(out).readline().startswith("# ") and len(back["auc"]) == 6
    for name in combo_grid.COLUMNS:
        assert np.array_equal(back[name], table[name]), name
    assert back["best"] == table["best"]
    assert combo_grid.main(argv + ["--both_strands"]) == 0
    fold = lambda path: kmer.normalize_counts(transform_kmers.fold_strands(fileIO.read_feature_file(path)[1]))   # noqa: E731
    folded = combo_grid.grid(fold(files[0]), fold(files[1]), [1, 3], [4, 9, 4], folds=3, seed=1)
    back = combo_grid.read_grid(out)
    for name in combo_grid.COLUMNS:
        assert np.array_equal(back[name], folded[name]), name
