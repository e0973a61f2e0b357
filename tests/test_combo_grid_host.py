"""CPU-only: the NumPy statement of a cell of the k_neighbors x k_clusters grid (tests/combo_grid_ref.py) against
scikit-learn, the oracle and -- for the parts that take fold ids of the caller's own -- a plain Python brute force, the inputs
of tests/test_gpu_combo_grid_shapes.py, and the host side of phamers_amd.combo_grid: argument checks that come before any device call,
the CSV, the three command lines' new options, and the new kernels' figures in the built library's code objects."""
import os
import re

import numpy as np
import pytest

from tests import combo_grid_ref as ref
from tests.helpers import REPO

FOLDS, SEED = 3, 0


# ---- the statement ---------------------------------------------------------------------------------------------------
def test_statement_votes_equal_scikit_learn_per_fold():
    from sklearn.neighbors import KNeighborsClassifier
    P, N = ref.blob_fixture()
    X = np.vstack((P, N))
    y = np.r_[np.ones(len(P)), np.zeros(len(N))]
    fold_of = ref.fold_ids(len(P), len(N), FOLDS, SEED)
    ks = (1, 2, 3, 4, 8)
    got = ref.knn_scores(P, N, FOLDS, SEED, ks)
    for i, k in enumerate(ks):
        want = np.empty(len(X))
        for f in range(FOLDS):
            out = fold_of == f
            pred = KNeighborsClassifier(n_neighbors=k, algorithm="brute").fit(X[~out], y[~out]).predict(X[out])
            want[out] = np.where(pred == 1, 1.0, -1.0)     # (an even split goes to the lower class, 0: -1)
        assert np.array_equal(got[i], want), k


def test_statement_kmeans_half_equals_the_oracle():
    from oracle import oracle
    P, N = ref.blob_fixture()
    X = np.vstack((P, N))
    fold_of = ref.fold_ids(len(P), len(N), FOLDS, SEED)
    rng = np.random.RandomState(3)
    cents = {f: (P[rng.choice(len(P), 5, replace=False)] + 0.01, N[rng.choice(len(N), 4, replace=False)] - 0.01) for f in range(FOLDS)}
    got = ref.kmeans_scores(P, N, FOLDS, SEED, cents)
    for f in range(FOLDS):
        rows = np.flatnonzero(fold_of == f)
        want = np.asarray(oracle.centroid_score_points(X[rows], cents[f][0], cents[f][1])).ravel()
        assert np.allclose(got[rows], want, rtol=1e-12, atol=1e-14)


def test_statement_ties_go_to_the_lower_index_and_leave_the_own_fold_out():
    X = np.array([[0.0], [1.0], [1.0], [-1.0], [5.0]])
    fold_of = np.array([0, 1, 2, 1, 0])
    is_pos = np.array([1, 0, 1, 1, 0], bool)
    bits = ref.neighbour_bits(X, fold_of, is_pos, 3)
    # row 0 (fold 0): rows 1, 2, 3 all at distance 1 -> index order 1, 2, 3; row 4 is of its own fold
    assert bits[0].tolist() == [False, True, True]
    assert ref.votes(bits, 1)[0] == -1.0 and ref.votes(bits, 2)[0] == -1.0 and ref.votes(bits, 3)[0] == 1.0
    # row 1 (fold 1): row 2 at distance 0, then row 0; row 3 is of its own fold
    assert bits[1].tolist() == [True, True, False]


def test_tie_fixture_has_duplicates_of_every_kind():
    P, N = ref.tie_fixture()
    X = np.vstack((P, N))
    fold_of = ref.fold_ids(40, 40, 4, SEED)
    same = (X[:, None, :] == X[None, :, :]).all(axis=2) & ~np.eye(80, dtype=bool)
    cls = np.r_[np.ones(40, bool), np.zeros(40, bool)]
    assert (same & (cls[:, None] != cls[None, :])).any()
    assert (same & (fold_of[:, None] != fold_of[None, :])).any()
    assert (same & (fold_of[:, None] == fold_of[None, :])).any()


# ---- the statement with fold ids of the caller's own (tests/test_gpu_combo_grid_shapes.py) ------------------------------
def _small_case():
    """13 integer-valued rows in 3 columns (every squared distance an exact small integer, many of them equal), four fold
    ids of which one holds nothing and one a single row."""
    rng = np.random.RandomState(5)
    X = rng.randint(0, 3, (13, 3)).astype(np.float64)
    X[7] = X[2]
    fold_of = np.array([0, 1, 0, 0, 1, 3, 0, 1, 0, 1, 0, 0, 1])
    is_pos = np.arange(13) % 3 != 1
    return X, fold_of, is_pos


def _d2(a, b):
    s = 0.0
    for x, y in zip(a, b):
        s += (float(x) - float(y)) * (float(x) - float(y))      # exact on the small case's integers
    return s


def test_neighbour_bits_and_votes_equal_a_plain_python_brute_force():
    X, fold_of, is_pos = _small_case()
    assert np.bincount(fold_of, minlength=4).tolist() == [7, 5, 0, 1]
    kmax = 6                                                    # the smallest train set: 13 - 7 rows
    bits = ref.neighbour_bits(X, fold_of, is_pos, kmax)
    assert bits.shape == (13, kmax) and bits.dtype == bool
    tied = 0
    for i in range(13):
        others = sorted((_d2(X[i], X[j]), j) for j in range(13) if fold_of[j] != fold_of[i])
        tied += len(set(d for d, _ in others[:kmax + 1])) <= kmax
        want = [bool(is_pos[j]) for _, j in others[:kmax]]
        assert bits[i].tolist() == want, i
        for k in range(1, kmax + 1):
            positive = sum(want[:k])
            assert ref.votes(bits, k)[i] == (1.0 if positive > k - positive else -1.0), (i, k)
    assert tied >= 10                                           # the order among equal distances is what is compared
    splits = [k for k in (2, 4, 6) if (2 * bits[:, :k].sum(axis=1) == k).any()]
    assert splits == [2, 4, 6]                                  # even splits occur, and go to -1.0 above


def test_kmeans_scores_for_equals_a_plain_python_brute_force():
    import math
    X, fold_of, _ = _small_case()
    rng = np.random.RandomState(6)
    cents = {f: (rng.randint(0, 3, (2 + f, 3)).astype(np.float64), rng.randint(0, 3, (3, 3)).astype(np.float64)) for f in range(4)}
    cents[0][0][1] = X[3]                                       # a held-out row of fold 0 as its own positive centroid
    cents[1][1][2] = X[4]                                       # and one of fold 1 as a negative centroid
    cents[1][0][:] = X[4] + 1.0
    got = ref.kmeans_scores_for(X, fold_of, cents)
    assert got.shape == (13,)
    eps = np.finfo(np.float64).eps
    for i in range(13):
        cp, cn = cents[int(fold_of[i])]
        ep = math.sqrt(min(_d2(X[i], c) for c in cp))
        en = math.sqrt(min(_d2(X[i], c) for c in cn))
        if ep + en == 0.0:
            assert np.isnan(got[i])
            continue
        want = math.tanh((en - ep) / (ep + en))
        assert abs(got[i] - want) <= 4 * eps * abs(want), i     # (two implementations of tanh)
    assert got[3] == np.tanh(1.0) and got[4] == np.tanh(-1.0)
    # the plan's own fold ids give kmeans_scores
    P, N = ref.blob_fixture()
    rng = np.random.RandomState(3)
    c3 = {f: (P[rng.choice(len(P), 5, replace=False)] + 0.01, N[rng.choice(len(N), 4, replace=False)] - 0.01) for f in range(FOLDS)}
    assert np.array_equal(ref.kmeans_scores_for(np.vstack((P, N)), ref.fold_ids(len(P), len(N), FOLDS, SEED), c3),
                          ref.kmeans_scores(P, N, FOLDS, SEED, c3))
    # a fold without a key, or without rows, is left out
    part = ref.kmeans_scores_for(X, fold_of, {0: cents[0], 2: cents[2]})
    assert np.array_equal(np.isnan(part), fold_of != 0) and np.array_equal(part[fold_of == 0], got[fold_of == 0])


def test_the_word_fixture_cannot_pass_with_a_narrower_word():
    """What tests/test_gpu_combo_grid_shapes.py asserts of its input, with the figures of this input."""
    X, fold_of, is_pos = ref.word_fixture()
    assert X.shape == (200, 17) and min(int((fold_of != f).sum()) for f in range(3)) == 130
    bits = ref.neighbour_bits(X, fold_of, is_pos, 64)
    for k in (1, 2, 31, 32, 33, 63, 64):
        assert set(ref.votes(bits, k).tolist()) == {-1.0, 1.0}, k
    assert int((bits.sum(axis=1) == 32).sum()) == 9
    assert int((ref.votes(bits, 63) != ref.votes(bits, 64)).sum()) == 3
    assert int(bits[:, 63].sum()) == 106


def test_blob_rows_at_other_widths_and_the_edge_fixtures():
    rng = np.random.RandomState(1)
    c = rng.rand(6, 20)
    assert np.array_equal(ref.blob_rows(1, 70), c[np.arange(70) % 6] + 0.02 * rng.randn(70, 20))     # D = 20: as before
    assert np.array_equal(ref.blob_rows(1, 70), ref.blob_fixture()[0]) and ref.blob_rows(4, 31, 257).shape == (31, 257)
    for M in (63, 64, 65, 127, 128, 129):
        held = np.bincount(ref.edge_folds(M), minlength=4)
        assert held[2] == 0 and held[3] == 1 and held[0] > held[1] > 1 and held.sum() == M and M - held.max() >= 5
        X, is_pos = ref.tie_rows(M)
        assert X.shape == (M, 8) and np.array_equal(X, np.round(X)) and 0 < is_pos.sum() < M
        if M > 80:
            assert np.array_equal(X[80:], X[:M - 80]) and np.array_equal(is_pos[80:], is_pos[:M - 80])


# ---- arguments: refused before any device call -------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    from phamers_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("a device call before the arguments were checked")
    monkeypatch.setattr(_lib, "get_context", refuse)
    monkeypatch.setattr(_lib, "ComboGrid", refuse)


def test_argument_errors_come_before_the_device(no_device, monkeypatch):
    from phamers_amd import combo_grid
    P, N = ref.blob_fixture()
    with pytest.raises(ValueError, match="at least one"):
        combo_grid.sweep(P, N, [], [], FOLDS, seed=SEED)
    with pytest.raises(ValueError, match="folds >= 2"):
        combo_grid.sweep(P, N, [3], [5], 1, seed=SEED)
    bad = P.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="Input contains NaN."):
        combo_grid.sweep(bad, N, [3], [5], FOLDS, seed=SEED)
    bad[3, 4] = np.inf
    with pytest.raises(ValueError, match="Input contains NaN."):
        combo_grid.sweep(P, bad, [3], [5], FOLDS, seed=SEED)
    with pytest.raises(ValueError, match="same number of columns"):
        combo_grid.sweep(P, N[:, :10], [3], [5], FOLDS, seed=SEED)
    # train sets: 46 or 47 positive + 50 negative rows; a class's smallest is 46
    for k in (0, -1, 65, 97):
        with pytest.raises(ValueError, match="k_neighbors"):
            combo_grid.sweep(P, N, [3, k], [5], FOLDS, seed=SEED)
    with pytest.raises(ValueError, match="k_neighbors"):
        combo_grid.sweep(P[:20], N[:20], [27], [], 3, seed=SEED)      # train sets of 26 or 27 rows
    for k in (0, 47):
        with pytest.raises(ValueError, match="k_clusters"):
            combo_grid.sweep(P, N, [3], [5, k], FOLDS, seed=SEED)
    with pytest.raises(ValueError, match="integers"):
        combo_grid.sweep(P, N, [2.5], [5], FOLDS, seed=SEED)
    with pytest.raises(ValueError, match="at least one k_neighbors and one k_clusters"):
        combo_grid.grid(P, N, [3], [], FOLDS, seed=SEED)
    monkeypatch.setenv("PHAMERS_KMEANS", "gpu")
    with pytest.raises(NotImplementedError):
        combo_grid.sweep(P, N, [3], [5], FOLDS, seed=SEED)


# ---- the CSV ---------------------------------------------------------------------------------------------------------
def _table():
    return {"k_neighbors": np.array([1.0, 1.0, 3.0, 3.0]), "k_clusters": np.array([2.0, 86.0, 2.0, 86.0]),
            "knn_auc": np.array([0.7, 0.7, 1.0 / 3.0, 1.0 / 3.0]), "kmeans_auc": np.array([0.1, 0.9, 0.1, 0.9]),
            "auc": np.array([0.25, 0.9500000000000001, 0.9500000000000001, 0.5]), "accuracy": np.array([0.5, 2.0 / 3.0, 0.75, 1.0]),
            "best": 1}


def test_grid_file_round_trip_and_best(tmp_path):
    from phamers_amd import combo_grid
    table, path = _table(), str(tmp_path / "grid.csv")
    args = combo_grid._parser().parse_args(["-pf", "p.csv", "-nf", "n.csv", "--k_neighbors", "1", "3", "--k_clusters", "2", "86",
                                            "-N", "5"])
    combo_grid.save_grid(path, table, args=args)
    lines = open(path).read().splitlines()
    assert lines[0].startswith("# ") and any("k_neighbors,k_clusters,knn_auc,kmeans_auc,auc,accuracy" in l for l in lines)
    data = [l for l in lines if not l.startswith("#")]
    assert data[1] == "1,86,0.7,0.9,0.9500000000000001,0.6666666666666666"
    back = combo_grid.read_grid(path)
    for name in combo_grid.COLUMNS:
        assert np.array_equal(back[name], table[name]), name
    assert back["best"] == 1                                       # the first of the two largest
    combo_grid.save_grid(path, {k: (v[:0] if k != "best" else None) for k, v in table.items()})
    assert combo_grid.read_grid(path)["best"] is None


# ---- the command lines -------------------------------------------------------------------------------------------------
def test_combo_grid_command_line():
    from phamers_amd import combo_grid
    a = combo_grid._parser().parse_args(["-data", "d", "--k_neighbors", "1", "3", "5", "--k_clusters", "20", "86", "-N", "20",
                                         "--seed", "4", "--both_strands", "-out", "t.csv"])
    assert (a.k_neighbors, a.k_clusters, a.N_fold, a.seed, a.both_strands, a.output_file) == ([1, 3, 5], [20, 86], 20, 4, True, "t.csv")
    b = combo_grid._parser().parse_args(["-pf", "p", "-nf", "n", "--k_neighbors", "3", "--k_clusters", "86", "-N", "2"])
    assert b.seed is None and not b.both_strands and b.output_file is None
    for argv in (["-data", "d", "--k_clusters", "86", "-N", "2"], ["-data", "d", "--k_neighbors", "3", "-N", "2"],
                 ["-data", "d", "--k_neighbors", "3", "--k_clusters", "86"], ["-data", "d", "-k", "3", "--k_clusters", "86", "-N", "2"]):
        with pytest.raises(SystemExit):
            combo_grid._parser().parse_args(argv)
    with pytest.raises(SystemExit):
        combo_grid.main(["--k_neighbors", "3", "--k_clusters", "86", "-N", "2"])


def test_validator_command_line_sets_the_validator_s_attributes():
    from phamers_amd import cross_validate, phamer
    parser = cross_validate._parser()
    plain = parser.parse_args(["-pf", "p", "-nf", "n"])
    assert not hasattr(plain, "k_neighbors") and not hasattr(plain, "k_clusters")
    v = cross_validate.cross_validator()
    phamer._apply_k_options(v, plain)
    assert (v.k_neighbors, v.k_clusters) == (3, 86)
    given = parser.parse_args(["-pf", "p", "-nf", "n", "--k_neighbors", "5", "--k_clusters", "40"])
    phamer._apply_k_options(v, given)
    assert (v.k_neighbors, v.k_clusters) == (5, 40)
    with pytest.raises(SystemExit):
        phamer._apply_k_options(v, parser.parse_args(["-pf", "p", "-nf", "n", "--k_clusters", "0"]))


def test_scorer_command_line_sets_the_scorer_s_attributes():
    from phamers_amd import phamer
    ap = phamer._parser()
    plain = ap.parse_args(["-in", "x", "-data", "d"])
    assert not hasattr(plain, "k_neighbors") and not hasattr(plain, "k_clusters")
    assert plain.kmer_length == 4
    s = phamer.phamer_scorer()
    phamer._apply_k_options(s, plain)
    assert (s.k_neighbors, s.k_clusters) == (3, 86)
    given = ap.parse_args(["-in", "x", "-data", "d", "-k", "5", "--k_neighbors", "7", "--k_clusters", "120"])
    assert given.kmer_length == 5                                   # -k is still the k-mer length
    phamer._apply_k_options(s, given)
    assert (s.k_neighbors, s.k_clusters) == (7, 120)
    # with the flags absent the argument summary stamped into the output files is what it was
    from phamers_amd import fileIO
    assert "k_neighbors" not in fileIO.generate_summary(plain) and "k_clusters" not in fileIO.generate_summary(plain)


# ---- the code objects ---------------------------------------------------------------------------------------------------
NEW_KERNELS = ("cg_centroid_kernel", "cg_pair_kernel", "cg_select_kernel", "cg_centroid_pass_kernel", "cg_fill_kernel",
               "cg_epilogue_kernel")
FOLD_ROW_KERNELS = ("kb_seed_dist_kernel", "kb_seed_choose_kernel", "kb_assign_kernel", "kb_update_kernel")


@pytest.fixture(scope="module")
def resources():
    from phamers_amd import _codeobj, _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _codeobj.kernel_resources(_lib.LIB_PATH)


def test_new_kernels_are_in_the_library_within_their_launch_bounds(resources):
    text = open(os.path.join(REPO, "phamers_amd", "csrc", "combo_grid.hip")).read()
    found = {}
    for kernel in NEW_KERNELS:
        assert re.search(r"__launch_bounds__\((256|CL_THREADS)\)\s+void " + kernel + r"\(", text), kernel
        hits = {name: r for name, r in resources.items() if kernel in name}
        assert len(hits) == 1, (kernel, sorted(hits))
        found.update(hits)
    for kernel in FOLD_ROW_KERNELS:                    # kmeans_batch.h's kernels as instantiated for the fold row source
        hits = {name: r for name, r in resources.items() if kernel in name and "KbFoldRows" in name}
        assert len(hits) == 1, (kernel, sorted(hits))
        found.update(hits)
    # 256 threads = one wave per SIMD at the least: 512 registers per lane (vector and accumulator together), no scratch
    for name, r in found.items():
        assert r["vgpr_spill_count"] == 0 and r["scratch_bytes"] == 0, (name, r)
        assert r["vgpr_count"] <= 512, (name, r)
    # the two pair passes keep at least four waves per SIMD
    for kernel in ("cg_pair_kernel", "cg_centroid_pass_kernel"):
        (r,) = [r for name, r in found.items() if kernel in name]
        assert r["vgpr_count"] <= 128, (kernel, r)
