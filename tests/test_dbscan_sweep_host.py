"""CPU: the DBSCAN parameter sweep without a device -- the restatement (tests/dbscan_sweep_ref.py) against scikit-learn and
against the fixture (tests/golden/dbscan_sweep.npz, tools/gen_golden_dbscan_sweep.py), the order of the records, the
argument checks of learning.dbscan_sweep / kdistances, and the CSV of phamers_amd.dbscan_grid."""
import itertools

import numpy as np
import pytest

from tests import cluster_ref, dbscan_sweep_ref, helpers

MIN_MARGIN = 1e-9


def _phage_rows():
    from oracle import oracle
    return oracle.normalize_counts(helpers.load_npz("ref_features.npz")["pos_counts"].astype(np.int64))


def _blobs_and_noise():
    """Three blobs of 35 points and 15 scattered points: n = 120, D = 3."""
    rng = np.random.RandomState(11)
    centres = np.array([[0.0, 0.0, 0.0], [3.0, 0.5, 1.0], [1.0, 4.0, -2.0]])
    X = np.vstack([c + 0.3 * rng.randn(35, 3) for c in centres] + [rng.uniform(-3, 6, (15, 3))])
    return X[rng.permutation(X.shape[0])]


def _against_scikit_learn(X, eps_values, min_samples_values):
    from sklearn.cluster import DBSCAN
    records = dbscan_sweep_ref.dbscan_sweep(X, eps_values, min_samples_values)
    cells = [(e, m) for e in eps_values for m in min_samples_values]
    assert [(r["eps"], r["min_samples"]) for r in records] == cells
    for r, (eps, m) in zip(records, cells):
        fit = DBSCAN(eps=eps, min_samples=m).fit(X)
        assert np.array_equal(r["labels"], fit.labels_), (eps, m)
        assert np.array_equal(r["core_sample_indices"], fit.core_sample_indices_), (eps, m)
        assert r["n_clusters"] == len(set(fit.labels_.tolist()) - {-1})
        assert r["n_core"] == len(fit.core_sample_indices_)
        assert r["n_noise"] == int(np.sum(fit.labels_ == -1))
        assert r["n_core"] + r["n_border"] + r["n_noise"] == X.shape[0]
        assert r["largest"] == (np.bincount(fit.labels_[fit.labels_ >= 0]).max() if r["n_clusters"] else 0)
    return records


def test_restatement_equals_scikit_learn_on_blobs_and_noise():
    X = _blobs_and_noise()
    assert X.shape == (120, 3)
    eps_values = (0.25, 0.4, 0.7)
    for eps in eps_values:
        assert cluster_ref.eps_margin(X, eps) >= MIN_MARGIN
    records = _against_scikit_learn(X, eps_values, (1, 3, 6, 121))
    assert len({r["n_clusters"] for r in records}) > 3            # the grid tells cells apart
    assert all(r["n_core"] == 0 and r["n_noise"] == 120 and r["largest"] == 0 for r in records if r["min_samples"] == 121)


def test_restatement_equals_scikit_learn_on_the_3_4_5_points():
    X = np.array([[0.0, 0.0], [3.0, 4.0], [6.0, 8.0]])
    assert np.array_equal(cluster_ref.pair_distances(X, X)[0], [0.0, 5.0, 10.0])    # exact: a pair AT eps = 5 is a neighbour
    records = _against_scikit_learn(X, (5.0,), (2, 3, 4))
    assert [r["n_clusters"] for r in records] == [1, 1, 0]
    assert [r["n_core"] for r in records] == [3, 1, 0] and [r["n_border"] for r in records] == [0, 2, 0]


@pytest.mark.parametrize("order", ["".join(p) for p in itertools.permutations("abp")])
def test_restatement_equals_scikit_learn_on_the_border_tie(order):
    X = cluster_ref.border_tie(order)
    assert cluster_ref.eps_margin(X, 0.9) >= MIN_MARGIN
    records = _against_scikit_learn(X, (0.9,), (4, 3))
    p = sum(1 if part == "p" else 4 for part in order[:order.index("p")])          # the row of the point between the clusters
    assert records[0]["n_clusters"] == 2 and records[0]["labels"][p] == 0 and p not in records[0]["core_sample_indices"]
    assert records[1]["n_clusters"] == 1 and p in records[1]["core_sample_indices"]     # core at 3: it bridges the two


def test_restatement_equals_the_fixture_on_its_corner_cells():
    g = helpers.load_npz("dbscan_sweep.npz")
    assert str(g["sklearn_version"]) and (g["eps_margin"] >= MIN_MARGIN).all()
    eps_values, ms_values = g["eps_values"], g["min_samples_values"]
    assert g["labels"].shape == (len(eps_values) * len(ms_values), 2255) and g["labels"].dtype == np.int16
    X = _phage_rows()
    for ie in (0, len(eps_values) - 1):
        for im in (0, len(ms_values) - 1):
            cell = ie * len(ms_values) + im
            record = dbscan_sweep_ref.dbscan_sweep(X, [eps_values[ie]], [ms_values[im]])[0]
            assert np.array_equal(record["labels"], g["labels"][cell]), cell
            for name in dbscan_sweep_ref.SUMMARY:
                assert record[name] == g[name][cell], (cell, name)


def test_restatement_keeps_cell_order_and_duplicates():
    X = _blobs_and_noise()[:40]
    records = dbscan_sweep_ref.dbscan_sweep(X, [0.7, 0.25, 0.7], [3, 1, 3])
    assert [(r["eps"], r["min_samples"]) for r in records] == [(e, m) for e in (0.7, 0.25, 0.7) for m in (3, 1, 3)]
    dbscan_sweep_ref.same_records([records[0]], [records[2]])
    dbscan_sweep_ref.same_records(records[:3], records[6:])


class _Stop(Exception):
    pass


def _refuse(*a, **k):
    raise _Stop()


@pytest.fixture
def no_device(monkeypatch):
    from phamers_amd import _lib
    monkeypatch.setattr(_lib, "get_context", _refuse)
    monkeypatch.setattr(_lib, "load", _refuse)
    monkeypatch.setattr(_lib, "DbscanRows", _refuse)


def test_sweep_keeps_cell_order_duplicates_and_passes(monkeypatch):
    """learning.dbscan_sweep over a stand-in for the device: the cells reach it in order, at most _cells_per_pass at a time,
    and every record is built from its own cell's outputs."""
    from phamers_amd import _lib, learning
    X = _blobs_and_noise()[:40]
    calls = []

    class FakeRows(object):
        def __init__(self, ctx, rows):
            assert np.array_equal(rows, X)

        def run(self, eps, min_samples, tiles_per_launch=0):
            calls.append((list(eps), list(min_samples), tiles_per_launch))
            out = {"labels": np.empty((len(eps), 40), dtype=np.int32), "coremask": np.zeros(40, dtype=np.uint64),
                   "n_clusters": np.empty(len(eps), dtype=np.uint64), "launches": np.array([1, 1, 1], dtype=np.uint32)}
            for c, (e, m) in enumerate(zip(eps, min_samples)):
                labels, core = cluster_ref.dbscan(X, e, m)
                out["labels"][c] = labels
                out["coremask"] |= core.astype(np.uint64) << np.uint64(c)
                out["n_clusters"][c] = labels.max() + 1
            return out

        def close(self):
            calls.append("closed")

    monkeypatch.setattr(_lib, "get_context", lambda: None)
    monkeypatch.setattr(_lib, "DbscanRows", FakeRows)
    eps_values, ms_values = [0.7, 0.25, 0.7], np.array([3, 1, 3])
    want = dbscan_sweep_ref.dbscan_sweep(X, eps_values, ms_values)
    details = {}
    got = learning.dbscan_sweep(X, eps_values, ms_values, _cells_per_pass=4, _tiles_per_launch=7, _details=details)
    dbscan_sweep_ref.same_records(got, want)
    assert all(r["route"] == "device" and r["labels"].dtype == np.int64 for r in got)
    assert [len(c[0]) for c in calls[:-1]] == [4, 4, 1] and calls[-1] == "closed" and all(c[2] == 7 for c in calls[:-1])
    assert details["passes"] == 3 and details["launches"] == [[1, 1, 1]] * 3
    assert calls[0][:2] == ([0.7, 0.7, 0.7, 0.25], [3, 1, 3, 3])
    assert "silhouette" not in got[0]


@pytest.mark.parametrize("eps_values, ms_values", [
    ([0.5, 0.0], [2]), ([0.5, -1.0], [2]), ([float("nan")], [2]), ([0.5, float("inf")], [2]),
    ([0.5], [2, 0]), ([0.5], [2, -3]), ([0.5], [2.0]), ([0.5], [True]), ([0.5], [2, 2.5]),
])
def test_bad_parameters_raise_before_any_device_work(no_device, eps_values, ms_values):
    from phamers_amd import learning
    X = _blobs_and_noise()[:20]
    with pytest.raises(ValueError, match="parameter of DBSCAN must be"):
        learning.dbscan_sweep(X, eps_values, ms_values)
    with pytest.raises(ValueError, match="parameter of DBSCAN must be"):       # the same message dbscan_fit gives
        learning.dbscan_fit(X, eps_values[-1], ms_values[-1])


def test_bad_data_and_empty_lists_need_no_device(no_device):
    from phamers_amd import learning
    X = _blobs_and_noise()[:20]
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="Input contains NaN"):
        learning.dbscan_sweep(bad, [0.5], [2])
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        learning.dbscan_sweep(bad, [0.5], [2])
    with pytest.raises(ValueError, match="Expected 2D array"):
        learning.dbscan_sweep(X[0], [0.5], [2])
    with pytest.raises(ValueError, match="0 sample"):
        learning.dbscan_sweep(X[:0], [0.5], [2])
    with pytest.raises(ValueError, match="_cells_per_pass"):
        learning.dbscan_sweep(X, [0.5], [2], _cells_per_pass=65)
    assert learning.dbscan_sweep(X, [], [2, 3]) == [] and learning.dbscan_sweep(X, [0.5], []) == []
    with pytest.raises(ValueError, match="parameter of DBSCAN must be"):       # a bad value beside an empty list still raises
        learning.dbscan_sweep(X, [], [0])


def test_kdistances_argument_errors(no_device):
    from phamers_amd import learning
    X = _blobs_and_noise()[:20]
    for k in (0, 29, -1):
        with pytest.raises(ValueError, match="not in 1..28"):
            learning.kdistances(X, k)
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        learning.kdistances(X[:5], 6)
    with pytest.raises(ValueError, match="2-D"):
        learning.kdistances(X[0], 1)
    bad = X.copy()
    bad[0, 0] = np.nan
    with pytest.raises(ValueError, match="Input contains NaN"):
        learning.kdistances(bad, 2)


def test_grid_csv_round_trip(tmp_path, monkeypatch):
    import argparse

    from phamers_amd import dbscan_grid, learning
    records = [{"eps": 0.004, "min_samples": 2, "n_clusters": 268, "n_core": 1257, "n_border": 0, "n_noise": 998, "largest": 61,
                "silhouette": 0.1 + 0.2},
               {"eps": 1.0 / 3.0, "min_samples": 10, "n_clusters": 0, "n_core": 0, "n_border": 0, "n_noise": 2255, "largest": 0,
                "silhouette": float("nan")}]
    seen = {}

    def fake_sweep(data, eps_values, min_samples_values, silhouettes=False):
        seen["args"] = (list(eps_values), list(min_samples_values), silhouettes)
        return [dict(r) for r in records] if silhouettes else [{k: v for k, v in r.items() if k != "silhouette"} for r in records]

    monkeypatch.setattr(learning, "dbscan_sweep", fake_sweep)
    for silhouettes in (True, False):
        table = dbscan_grid.grid(np.zeros((3, 2)), [0.004, 1.0 / 3.0], [2, 10], silhouettes=silhouettes)
        assert seen["args"] == ([0.004, 1.0 / 3.0], [2, 10], silhouettes)
        assert set(table) == set(dbscan_grid.COLUMNS)
        if not silhouettes:
            assert np.isnan(table["silhouette"]).all()
        path = str(tmp_path / ("grid_%d.csv" % silhouettes))
        dbscan_grid.save_grid(path, table, args=argparse.Namespace(features_file="x.csv", eps=[0.004]) if silhouettes else None)
        lines = open(path).read().splitlines()
        assert lines[0].startswith("# DBSCAN parameter grid: eps,min_samples,n_clusters,n_core,n_border,n_noise,largest,silhouette")
        assert all(line.startswith("# ") for line in lines[:-2]) and not lines[-1].startswith("#")
        assert lines[-2].startswith("0.004,2,268,1257,0,998,61,")
        back = dbscan_grid.read_grid(path)
        for name in dbscan_grid.COLUMNS:
            assert back[name].dtype == table[name].dtype
            assert np.array_equal(back[name], table[name], equal_nan=True), name      # repr round-trips every float


# ---- the inputs of tests/test_gpu_dbscan_sweep_shapes.py: what that file assumes of them, asserted without a device --------
def test_groups_restates_cl_groups():
    g = dbscan_sweep_ref.groups
    assert g(256, 45, 45) == 45 and g(256, 46, 46) == 45 and g(256, 90, 90) == 23          # T^2 <= 8 cus: one tile per group
    assert g(256, 2048, 7) == 1 and g(256, 5000, 7) == 1 and g(256, 1, 3) == 3 and g(256, 3, 4000) == 683
    assert max(n for n in range(1, 4000) if g(256, -(-n // 64), -(-n // 64)) == -(-n // 64)) == 2880
    assert dbscan_sweep_ref.group_tiles(90, 23).count(4) == 21 and sum(dbscan_sweep_ref.group_tiles(90, 23)) == 90


@pytest.mark.parametrize("cus", [32, 256, 304])
def test_scattered_lattice_meets_the_conditions_of_its_cases(cus):
    """Cases 1 and 2 of the shapes file at three sizes of device: groups of several tiles (unevenly many from 256 compute
    units on), hundreds of pairs exactly at every eps, and with min_samples 6 and 12 both row-index sides proper subsets
    spanning more tiles than one group walks.  The eight cells of case 2 have 8 distinct cluster counts on the 256 compute
    units of an MI355X, which is what the device test asserts; 7 on 32 units and 6 on 304."""
    R = dbscan_sweep_ref
    T, n = R.lattice_tiles(cus), R.lattice_rows(cus)
    assert (T, n) == {32: (32, 2025), 256: (90, 5737), 304: (98, 6249)}[cus]
    X = R.scattered_lattice(n, 41)
    assert X.shape == (n, 2) and np.array_equal(X, R.scattered_lattice(n, 41))
    G = R.groups(cus, T, T)
    assert 1 < G < T and min(R.group_tiles(T, G)) >= 2
    if cus >= 256:
        assert len(set(R.group_tiles(T, G))) > 1
    assert min(R.pairs_exactly_at(X, R.LATTICE_EPS)) >= 900
    records = R.sweep_cells(X, [(e, m) for e in R.LATTICE_EPS for m in (6, 12)])
    nu, nb = R.core_somewhere(records, n)
    assert 20 * R.TILE < nu < n and 20 * R.TILE < nb < n
    Tq, Tu = -(-nb // R.TILE), -(-nu // R.TILE)
    assert Tq * Tu > 8 * cus and R.groups(cus, Tq, Tu) < Tu
    assert len({r["n_clusters"] for r in records}) >= {32: 7, 256: 8, 304: 6}[cus]
    assert max(R.borders_between_clusters(X, r) for r in records) >= 1
    if cus == 256:
        assert (nu, nb, R.groups(cus, Tq, Tu), Tu) == (4948, 3012, 43, 78)
    # with min_samples = 1 and n + 1 beside them every row is on both sides
    assert R.core_somewhere(R.sweep_cells(X, [(0.5, 1), (0.5, n + 1)]), n) == (n, n)


def test_pairs_exactly_at_counts_like_the_distance_matrix():
    X = dbscan_sweep_ref.scattered_lattice(700, 3)
    d = cluster_ref.pair_distances(X, X)[np.triu_indices(700, 1)]
    eps_values = dbscan_sweep_ref.LATTICE_EPS + (1.25,)                 # 1.25: (3, 4) and (5, 0) offsets
    assert dbscan_sweep_ref.pairs_exactly_at(X, eps_values) == [int(np.count_nonzero(d == e)) for e in eps_values]


def test_dbscan_cells_equals_dbscan_on_the_lattice():
    """The reference of the large cases against the plain one, with pairs exactly at eps and border ties."""
    X = dbscan_sweep_ref.scattered_lattice(900, 5)
    cells = [(e, m) for e in dbscan_sweep_ref.LATTICE_EPS for m in (1, 6, 901, 12)]
    want = dbscan_sweep_ref.dbscan_sweep(X, dbscan_sweep_ref.LATTICE_EPS, (1, 6, 901, 12))
    dbscan_sweep_ref.same_records(dbscan_sweep_ref.sweep_cells(X, cells), want)
    assert max(dbscan_sweep_ref.borders_between_clusters(X, r) for r in want) >= 1


def test_clump_cells_fill_every_bin_at_every_number_of_thresholds():
    R = dbscan_sweep_ref
    X = R.clumps()
    cells = R.clump_cells(X)
    assert X.shape == (150, 3) and len(cells) == 64 and len({e for e, _ in cells}) == 64
    eps = np.array([e for e, _ in cells])
    assert (np.diff(eps) < 0).any() and (np.diff(eps) > 0).any()                      # not sorted
    assert sum(1 for e in eps if 16 * e * e != round(16 * e * e)) >= 16               # square roots that were rounded
    assert {m for _, m in cells} == {1, 2, 3, 4, 6, 9, 151, 2 ** 40}
    for E in range(1, 65):
        counts = R.bin_counts(X, eps[:E])
        assert len(counts) == E + 1 and counts[:E].min() >= 1 and counts[E] >= 1, E
    records = R.sweep_cells(X, cells)
    R.same_records(records, [R.dbscan_sweep(X, [e], [m])[0] for e, m in cells])
    assert len({tuple(r[k] for k in R.SUMMARY) for r in records}) >= 20
    assert all(r["n_core"] == 0 for r in records if r["min_samples"] > 150)
    assert any(r["n_border"] for r in records)
    for thresholds in (32, 2):                                                        # 64 cells on fewer thresholds
        some = R.cells_64(cells, thresholds)
        assert len(some) == 64 and len({e for e, _ in some}) == thresholds
        records = R.sweep_cells(X, some)
        assert len({tuple(r[k] for k in R.SUMMARY) for r in records}) >= 20 and sum(1 for r in records if r["n_border"]) >= 20


@pytest.mark.parametrize("D", [33, 100])
def test_general_rows_keep_their_margin_in_extended_precision(D):
    R = dbscan_sweep_ref
    X = R.blobs(130, D, D)
    d = R.extended_distances(X)
    assert d.dtype == np.longdouble and np.array_equal(d, d.T) and (np.diag(d) == 0).all()
    eps_values = R.midpoint_eps(d)
    assert len(set(eps_values)) == 4 and R.relative_margin(d, eps_values) >= R.MARGIN
    assert (D + 3) * 2.0 ** -53 * 64 <= R.MARGIN
    records = R.cells_of_distances(d, [(e, m) for e in eps_values for m in (1, 3, 5, 9)])
    R.same_records(records, R.dbscan_sweep(X, eps_values, (1, 3, 5, 9)))              # float64 decides the same: the margin
    assert len({r["n_clusters"] for r in records}) >= 4 and any(r["n_border"] for r in records)


def test_rows_with_infinities_are_nobodys_neighbours():
    R = dbscan_sweep_ref
    X, where = R.rows_with_infinities()
    assert X.shape == (107, 4) and not np.isnan(X).any() and np.array_equal(np.flatnonzero(~np.isfinite(X).all(axis=1)), where)
    with np.errstate(invalid="ignore"):
        d = cluster_ref.pair_distances(X, X)
        records = R.dbscan_sweep(X, [0.4, 0.8], [1, 4])
    assert np.isnan(d[where, where]).all() and np.isnan(d[where[0], where[1]]) and np.isinf(d[where[0], where[2]])
    assert not (d[where] <= 1e300).any()
    for r in records:
        assert (r["labels"][where] == -1).all() and not set(where) & set(r["core_sample_indices"])
    finite = np.delete(np.arange(107), where)
    for r, (e, m) in zip(records, [(e, m) for e in (0.4, 0.8) for m in (1, 4)]):      # the other rows: as without them
        labels, core = cluster_ref.dbscan(X[finite], e, m)
        assert np.array_equal(r["labels"][finite], labels) and np.array_equal(r["core_sample_indices"], finite[core])
    assert records[0]["n_core"] == 100 and records[0]["n_noise"] == 7 and 0 < records[1]["n_core"] < 100
