"""GPU: the DBSCAN eps x min_samples sweep (dbscan_sweep.hip, learning.dbscan_sweep) against scikit-learn's labels on the
phage rows (tests/golden/dbscan_sweep.npz, tools/gen_golden_dbscan_sweep.py), against the single-cell path (learning.dbscan_fit)
and against the NumPy restatement (tests/dbscan_sweep_ref.py).  Bar: labels, core points and summaries identical."""
import itertools

import numpy as np
import pytest

from tests import cluster_ref, dbscan_sweep_ref, helpers

pytestmark = pytest.mark.gpu
same = dbscan_sweep_ref.same_records


@pytest.fixture(scope="module")
def phage():
    from oracle import oracle
    X = oracle.normalize_counts(helpers.load_npz("ref_features.npz")["pos_counts"].astype(np.int64))
    X.setflags(write=False)
    return X


@pytest.fixture(scope="module")
def golden():
    return helpers.load_npz("dbscan_sweep.npz")


@pytest.fixture(scope="module")
def phage_records(phage, golden):
    """The fixture's 28 cells in one sweep (shared, read only)."""
    from phamers_amd import learning
    return learning.dbscan_sweep(phage, golden["eps_values"], golden["min_samples_values"])


def _blobs(n, D, seed):
    rng = np.random.RandomState(seed)
    centres = 3.0 * rng.randn(4, D)
    X = centres[rng.randint(0, 4, n)] + 0.35 * rng.randn(n, D)
    X[rng.rand(n) < 0.1] += 2.0 * rng.randn(D)
    return X


def test_golden_cells_equal_scikit_learn_and_the_single_cell_path(phage, golden, phage_records):
    from phamers_amd import learning
    cells = [(float(e), int(m)) for e in golden["eps_values"] for m in golden["min_samples_values"]]
    assert len(phage_records) == 28 == len(cells)
    for c, (record, (eps, m)) in enumerate(zip(phage_records, cells)):
        assert (record["eps"], record["min_samples"], record["route"]) == (eps, m, "device")
        assert record["labels"].dtype == np.int64 and np.array_equal(record["labels"], golden["labels"][c]), (eps, m)
        for name in dbscan_sweep_ref.SUMMARY:
            assert record[name] == golden[name][c], (eps, m, name)
        labels, core = learning.dbscan_fit(phage, eps, m)
        assert np.array_equal(record["labels"], labels) and np.array_equal(record["core_sample_indices"], core), (eps, m)


def _dyadic_points(n, D, seed):
    """Seeded points on a grid of quarters around four centres: every squared distance is exact in float64, in any order."""
    rng = np.random.RandomState(seed)
    centres = 2.0 * rng.randint(0, 4, (4, D))
    return centres[rng.randint(0, 4, n)] + 0.25 * rng.randint(0, 3, (n, D))


@pytest.mark.parametrize("D", [1, 15, 16, 17])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 200])
def test_shapes_against_the_restatement(n, D):
    from phamers_amd import learning
    X = _dyadic_points(n, D, 100 * n + D)
    d = cluster_ref.pair_distances(X, X)
    nonzero = np.sort(d[d > 0])
    # an eps below the smallest non-zero distance (0.25), and two that ARE pair distances (exact ties) where there are any
    eps_values = [0.125] + ([float(nonzero[len(nonzero) // 10]), float(nonzero[(2 * len(nonzero)) // 5])] if len(nonzero) else [0.5, 2.0])
    ms_values = [2, n + 1, 4]
    got = learning.dbscan_sweep(X, eps_values, ms_values)
    same(got, dbscan_sweep_ref.dbscan_sweep(X, eps_values, ms_values))
    for r in got:
        if r["min_samples"] == n + 1:
            assert r["n_core"] == 0 and r["n_clusters"] == 0 and r["n_noise"] == n and (r["labels"] == -1).all()
    if n > 2:
        assert len({r["n_clusters"] for r in got}) > 1
    # every cell at n + 1: no row is core anywhere, the union and border passes have nothing to do
    details = {}
    none = learning.dbscan_sweep(X, eps_values, [n + 1], _details=details)
    assert all(r["n_noise"] == n and r["core_sample_indices"].size == 0 for r in none)
    assert details["launches"][0][1:] == [0, 0]


@pytest.mark.parametrize("bridge_first", [False, True])
def test_a_row_that_is_not_core_does_not_bridge(bridge_first):
    """Two groups of five joined only through a point with three neighbours (itself and one row of each group): core at
    min_samples = 2, where it makes one cluster of everything, and a border point at 4, where the groups stay apart and it
    takes the smaller of their labels.  Both cells in one call: what the per-cell core mask is for."""
    from phamers_amd import learning
    a = np.array([[0.1 * i, 0.0] for i in range(5)])
    b = a + [2.3, 0.0]
    p = np.array([[1.35, 0.0]])
    X = np.vstack([p, b, a] if bridge_first else [b, a, p])
    ip = 0 if bridge_first else 10
    got = learning.dbscan_sweep(X, [1.0], [2, 4])
    same(got, dbscan_sweep_ref.dbscan_sweep(X, [1.0], [2, 4]))
    assert got[0]["n_clusters"] == 1 and (got[0]["labels"] == 0).all() and got[0]["n_core"] == 11
    assert got[1]["n_clusters"] == 2 and got[1]["n_core"] == 10 and got[1]["n_border"] == 1
    assert ip not in got[1]["core_sample_indices"] and got[1]["labels"][ip] == 0
    others = np.delete(got[1]["labels"], ip)
    assert np.array_equal(others, [0] * 5 + [1] * 5)


def test_pairs_at_eps_and_border_ties():
    from phamers_amd import learning
    X = np.array([[0.0, 0.0], [3.0, 4.0], [6.0, 8.0]])
    eps_values, ms_values = [4.999, 5.0, 5.001], [2, 3]
    got = learning.dbscan_sweep(X, eps_values, ms_values)
    same(got, dbscan_sweep_ref.dbscan_sweep(X, eps_values, ms_values))
    assert [r["n_clusters"] for r in got] == [0, 0, 1, 1, 1, 1]            # d = 5 = eps: neighbours
    assert [r["n_core"] for r in got] == [0, 0, 3, 1, 3, 1]
    for order in ("".join(p) for p in itertools.permutations("abp")):
        X = cluster_ref.border_tie(order)
        got = learning.dbscan_sweep(X, [0.9], [4, 3])
        same(got, dbscan_sweep_ref.dbscan_sweep(X, [0.9], [4, 3]))
        ip = sum(1 if part == "p" else 4 for part in order[:order.index("p")])
        assert got[0]["n_clusters"] == 2 and got[0]["labels"][ip] == 0 and got[0]["n_border"] == 1, order


def test_a_cell_does_not_depend_on_its_company():
    from phamers_amd import learning
    X = _blobs(150, 5, 3)
    eps_values, ms_values = [0.9, 0.5, 1.4, 0.7], [3, 1, 8]
    base = learning.dbscan_sweep(X, eps_values, ms_values)
    same(base, dbscan_sweep_ref.dbscan_sweep(X, eps_values, ms_values))
    assert len({r["n_clusters"] for r in base}) > 3
    cells = [(e, m) for e in eps_values for m in ms_values]
    for record, (e, m) in zip(base, cells):
        same(learning.dbscan_sweep(X, [e], [m]), [record])                              # alone
    twice = learning.dbscan_sweep(X, [0.9, 0.9], [3, 8, 3])                             # listed twice
    same(twice, [base[0], base[2], base[0]] * 2)
    same(learning.dbscan_sweep(X, eps_values[::-1], ms_values[::-1])[::-1], base)       # reversed
    details = {}
    same(learning.dbscan_sweep(X, eps_values, ms_values, _cells_per_pass=3, _details=details), base)
    assert details["passes"] == 4
    # 65 cells: two passes at the default
    many_eps = [0.4 + 0.1 * i for i in range(13)]
    many_ms = [1, 3, 5, 8, 3]
    details = {}
    many = learning.dbscan_sweep(X, many_eps, many_ms, _details=details)
    assert len(many) == 65 and details["passes"] == 2
    same(many, learning.dbscan_sweep(X, many_eps, many_ms, _cells_per_pass=7))
    same(many[60:], dbscan_sweep_ref.dbscan_sweep(X, many_eps[12:], many_ms))            # the second pass's cells
    for i in (0, 31, 63, 64):
        same(learning.dbscan_sweep(X, [many[i]["eps"]], [many[i]["min_samples"]]), [many[i]])


def test_past_one_launch_per_stage():
    """n = 200: a chain of 150 points a unit apart, its rows scattered over all four tiles, and 50 isolated points; one tile
    per launch.  The cell at min_samples = n + 1 makes every row a border candidate of the other cells' pass."""
    from phamers_amd import learning
    rng = np.random.RandomState(8)
    X = np.zeros((200, 2))
    X[:150, 0] = np.arange(150)
    X[150:, 0] = 4.0 * np.arange(50)
    X[150:, 1] = 64.0
    X = X[rng.permutation(200)]
    eps_values, ms_values = [1.0, 0.5, 4.0], [3, 201, 2]
    details, small = {}, {}
    base = learning.dbscan_sweep(X, eps_values, ms_values, _details=details)
    got = learning.dbscan_sweep(X, eps_values, ms_values, _tiles_per_launch=1, _details=small)
    assert details["launches"] == [[1, 1, 1]]
    assert all(k >= 4 for k in small["launches"][0]), small
    same(got, base)
    same(got, dbscan_sweep_ref.dbscan_sweep(X, eps_values, ms_values))
    assert got[0]["n_clusters"] == 1 and got[0]["largest"] == 150 and got[0]["n_border"] == 2 and got[0]["n_noise"] == 50
    assert got[8]["n_clusters"] == 2 and got[8]["n_noise"] == 0


def test_every_pair_an_edge_in_all_64_cells():
    from phamers_amd import learning
    X = _blobs(129, 7, 5)
    top = float(cluster_ref.pair_distances(X, X).max())
    eps_values = [top * (1.5 + 0.25 * i) for i in range(8)]
    details = {}
    got = learning.dbscan_sweep(X, eps_values, [1] * 8, _details=details)
    assert len(got) == 64 and details["passes"] == 1
    for r in got:
        assert (r["labels"] == 0).all() and np.array_equal(r["core_sample_indices"], np.arange(129))
        assert (r["n_clusters"], r["n_core"], r["n_border"], r["n_noise"], r["largest"]) == (1, 129, 0, 0, 129)


def test_kdistances_count_the_core_rows(phage, golden, phage_records):
    from phamers_amd import learning
    kd = {int(m): learning.kdistances(phage, int(m)) for m in golden["min_samples_values"] if m <= 10}
    assert len(kd) == 4
    for m, curve in kd.items():
        assert curve.shape == (2255,) and (np.diff(curve) >= 0).all()
    assert (kd[2] <= kd[3]).all() and (kd[3] <= kd[5]).all()
    for record in phage_records:
        assert record["n_core"] == np.count_nonzero(kd[record["min_samples"]] <= record["eps"]), (record["eps"], record["min_samples"])


def test_silhouettes_of_the_clustered_rows():
    from phamers_amd import learning
    X = _blobs(150, 5, 3)
    eps_values, ms_values = [0.9, 1.4, 40.0], [3]
    plain = learning.dbscan_sweep(X, eps_values, ms_values)
    got = learning.dbscan_sweep(X, eps_values, ms_values, silhouettes=True)
    same(got, plain)
    assert all("silhouette" not in r for r in plain)
    for r in got[:2]:
        clustered = r["labels"] >= 0
        assert r["n_clusters"] >= 2 and 0 < r["n_noise"]
        want = learning.silhouette_score(X[clustered], r["labels"][clustered])
        assert isinstance(r["silhouette"], float) and r["silhouette"] == want             # bit for bit
        ref = float(np.mean(cluster_ref.silhouettes(X[clustered], r["labels"][clustered])))
        assert abs(r["silhouette"] - ref) <= 1e-12
    assert got[2]["n_clusters"] == 1 and np.isnan(got[2]["silhouette"])


def test_command_line_writes_the_grid(tmp_path):
    from phamers_amd import dbscan_grid, fileIO, kmer, learning
    counts = helpers.load_npz("ref_features.npz")["pos_counts"][:300].astype(np.int64)
    features = str(tmp_path / "phage_features.csv")
    fileIO.save_counts(counts, ["p%d" % i for i in range(300)], features)
    out = str(tmp_path / "grid.csv")
    assert dbscan_grid.main(["-in", features, "-out", out, "--eps", "0.01", "0.02", "--min_samples", "2", "5", "--silhouettes"]) == 0
    table = dbscan_grid.read_grid(out)
    records = learning.dbscan_sweep(kmer.normalize_counts(counts), [0.01, 0.02], [2, 5], silhouettes=True)
    assert len(records) == 4 and len({r["n_clusters"] for r in records}) > 1
    for name in dbscan_grid.COLUMNS:
        assert np.array_equal(table[name], np.array([r[name] for r in records]), equal_nan=True), name
    assert open(out).readline().startswith("# DBSCAN parameter grid: eps,min_samples,")
    # the default file name, in the working directory
    import os
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        assert dbscan_grid.main(["-in", features, "--eps", "0.02", "--min_samples", "5"]) == 0
        plain = dbscan_grid.read_grid(str(tmp_path / "phage_features_dbscan.csv"))
    finally:
        os.chdir(cwd)
    assert plain["n_clusters"][0] == records[3]["n_clusters"] and np.isnan(plain["silhouette"]).all()


def test_library_refuses_what_phk_dbscan_refuses():
    """The C entry's own checks (learning.dbscan_sweep raises before it gets there): eps finite and > 0, min_samples >= 1,
    1 <= cells <= 64, NaN rows."""
    from phamers_amd import _lib
    ctx = _lib.get_context()
    X = _blobs(70, 3, 1)
    rows = _lib.DbscanRows(ctx, X)
    try:
        for eps, ms in (([0.5, 0.0], [2, 2]), ([float("inf")], [2]), ([float("nan")], [2]), ([-1.0], [2]), ([0.5], [0]),
                        ([], []), ([0.5] * 65, [2] * 65)):
            with pytest.raises(_lib.PhkError) as e:
                rows.run(eps, ms)
            assert e.value.code == _lib.PHK_ERR_ARG, (eps, ms)
        out = rows.run([0.5] * 64, [2] * 64)                      # the handle is still good, 64 cells are allowed
        assert (out["labels"] == out["labels"][0]).all() and len(set(out["n_clusters"].tolist())) == 1
    finally:
        rows.close()
    bad = X.copy()
    bad[69, 2] = np.nan
    with pytest.raises(_lib.PhkError) as e:
        _lib.DbscanRows(ctx, bad)
    assert e.value.code == _lib.PHK_ERR_NAN
