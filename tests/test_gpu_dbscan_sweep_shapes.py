"""The DBSCAN sweep (dbscan_sweep.hip) past the shapes of tests/test_gpu_dbscan_sweep.py: column groups that walk several
tiles, evenly and unevenly many (the LDS histogram and the LDS minima carried from tile to tile), launches that start at a
later query block with such groups, both row-index sides proper subsets over tens of tiles, every number of thresholds from
1 to 64 on cells in any order with any pairing, 64 cells on 64, 32 and 2 thresholds (the largest LDS layouts), min_samples
past 2^32, eps values that are adjacent doubles, general rows at D = 33 and 100, and rows holding infinities.

Bar: labels, core rows, the five summary numbers and n_clusters identical to the reference.  No tolerance: dyadic rows
(every squared distance exact in float64, pairs exactly at eps included), or general rows decided in np.longdouble with
every |d - eps| >= 2^-40 eps.  tests/dbscan_sweep_ref.py generates the inputs; what a case needs of its inputs is asserted
here before the device is asked, and in tests/test_dbscan_sweep_host.py without one."""
import subprocess
import sys

import numpy as np
import pytest

from tests import dbscan_sweep_ref as ref

pytestmark = pytest.mark.gpu
same = ref.same_records


@pytest.fixture(scope="module")
def compute_units():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked once in a child process: torch's HIP runtime has to
    be the first one initialised in its process, and this one opens the device through libphamers_hip.so."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[-1])


# ---- 1, 2. the scattered lattice: groups of several tiles -------------------------------------------------------------------
LATTICE_MS = (1, 6, None, 12)                 # None: n + 1


@pytest.fixture(scope="module")
def lattice(compute_units):
    """The rows, and the reference of the 16 cells once (shared, read only)."""
    assert 1 <= compute_units <= 1024
    T, n = ref.lattice_tiles(compute_units), ref.lattice_rows(compute_units)
    X = ref.scattered_lattice(n, 41)
    X.setflags(write=False)
    ms_values = [n + 1 if m is None else m for m in LATTICE_MS]
    cells = [(e, m) for e in ref.LATTICE_EPS for m in ms_values]
    return {"T": T, "n": n, "X": X, "ms": ms_values, "cells": cells, "want": ref.sweep_cells(X, cells)}


def test_groups_of_several_tiles_with_every_row_on_both_sides(compute_units, lattice):
    from phamers_amd import learning
    T, n, X, want = lattice["T"], lattice["n"], lattice["X"], lattice["want"]
    assert n == 64 * T - 23 and -(-n // 64) == T
    G = ref.groups(compute_units, T, T)
    tiles = ref.group_tiles(T, G)
    assert G < T and min(tiles) >= 2 and len(set(tiles)) > 1, (G, T)          # several tiles a group, unevenly many
    assert min(ref.pairs_exactly_at(X, ref.LATTICE_EPS)) >= 100
    assert ref.core_somewhere(want, n) == (n, n)                               # U and B are both every row
    assert len({r["n_clusters"] for r in want}) >= 8
    details = {}
    got = learning.dbscan_sweep(X, ref.LATTICE_EPS, lattice["ms"], _details=details)
    assert details["launches"] == [[1, 1, 1]]
    same(got, want)
    # three query blocks a launch: launches that start at a later query block, with groups of several tiles
    split = {}
    again = learning.dbscan_sweep(X, ref.LATTICE_EPS, lattice["ms"], _tiles_per_launch=3 * T, _details=split)
    assert split["launches"] == [[-(-T // 3)] * 3], split
    same(again, got)


def test_groups_of_several_tiles_with_proper_subsets_on_both_sides(compute_units, lattice):
    from phamers_amd import learning
    n, X = lattice["n"], lattice["X"]
    want = [r for r in lattice["want"] if r["min_samples"] in (6, 12)]
    assert len(want) == 8
    nu, nb = ref.core_somewhere(want, n)
    assert nu < n and nb < n
    Tq, Tu = -(-nb // 64), -(-nu // 64)
    assert Tq * Tu > 8 * compute_units and ref.groups(compute_units, Tq, Tu) < Tu
    assert len({r["n_clusters"] for r in want}) >= 8
    assert max(ref.borders_between_clusters(X, r) for r in want) >= 1
    got = learning.dbscan_sweep(X, ref.LATTICE_EPS, [6, 12])
    same(got, want)
    split = {}
    again = learning.dbscan_sweep(X, ref.LATTICE_EPS, [6, 12], _tiles_per_launch=5 * Tu, _details=split)
    assert split["launches"][0][1:] == [-(-Tu // 5), -(-Tq // 5)] and min(split["launches"][0]) > 1, split
    same(again, got)


# ---- 3, 4. threshold tables ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clumps():
    """150 dyadic rows, 64 cells on 64 thresholds in shuffled order, each cell's reference by cluster_ref.dbscan."""
    X = ref.clumps()
    X.setflags(write=False)
    cells = ref.clump_cells(X)
    return {"X": X, "cells": cells, "want": [ref.dbscan_sweep(X, [e], [m])[0] for e, m in cells]}


@pytest.fixture(scope="module")
def clump_rows(clumps):
    """The rows resident on the device, and every cell alone as the tests ask for it."""
    from phamers_amd import _lib
    rows = _lib.DbscanRows(_lib.get_context(), clumps["X"])
    alone = {}

    def single(cell):
        if cell not in alone:
            alone[cell] = ref.records_of_run(rows.run([cell[0]], [cell[1]]), [cell])[0]
        return alone[cell]

    yield rows, single
    rows.close()


def test_every_number_of_thresholds(clumps, clump_rows):
    from phamers_amd import learning
    X, cells, want = clumps["X"], clumps["cells"], clumps["want"]
    rows, _ = clump_rows
    assert len(cells) == 64 and {m for _, m in cells} >= {151, 2 ** 40}
    for E in range(1, 65):
        counts = ref.bin_counts(X, [e for e, _ in cells[:E]])
        assert len(counts) == E + 1 and counts.min() >= 1, E                  # E thresholds, a pair in every bin and beyond
    assert len({tuple(r[k] for k in ref.SUMMARY) for r in want}) >= 20
    for E in range(1, 65):
        out = rows.run([e for e, _ in cells[:E]], [m for _, m in cells[:E]])
        assert out["launches"].tolist()[0] == 1, E
        try:
            same(ref.records_of_run(out, cells[:E]), want[:E])
        except AssertionError as err:
            raise AssertionError("with %d thresholds: %s" % (E, err))
    for (eps, m), record in zip(cells, want):
        labels, core = learning.dbscan_fit(X, eps, m)
        assert np.array_equal(labels, record["labels"]) and np.array_equal(core, record["core_sample_indices"]), (eps, m)


@pytest.mark.parametrize("tiles_per_launch", [0, 1])
@pytest.mark.parametrize("thresholds", [64, 32, 2])
def test_64_cells_equal_their_single_cell_runs(clumps, clump_rows, thresholds, tiles_per_launch):
    rows, single = clump_rows
    cells = clumps["cells"] if thresholds == 64 else ref.cells_64(clumps["cells"], thresholds)
    out = rows.run([e for e, _ in cells], [m for _, m in cells], tiles_per_launch)
    assert (out["launches"] > 1).all() if tiles_per_launch else out["launches"].tolist() == [1, 1, 1]
    got = ref.records_of_run(out, cells)
    same(got, [single(cell) for cell in cells])
    assert len({tuple(r[k] for k in ref.SUMMARY) for r in got}) >= 20 and any(r["n_border"] for r in got)
    if thresholds == 64:
        same(got, clumps["want"])


# ---- 5. adjacent doubles ---------------------------------------------------------------------------------------------------------
def test_eps_values_that_are_adjacent_doubles():
    from phamers_amd import learning
    X = np.array([[0.0, 0.0], [3.0, 4.0], [6.0, 8.0]])
    eps_values = [float(np.nextafter(5.0, 0.0)), 5.0, float(np.nextafter(5.0, np.inf))]
    assert eps_values[0] < eps_values[1] < eps_values[2] and eps_values[2] - eps_values[0] < 2e-15
    got = learning.dbscan_sweep(X, eps_values, [2, 3])
    assert [r["n_core"] for r in got] == [0, 0, 3, 1, 3, 1]
    same(got, ref.dbscan_sweep(X, eps_values, [2, 3]))


# ---- 6. general rows against extended precision ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [33, 100])
def test_general_rows_against_extended_precision(D):
    from phamers_amd import learning
    X = ref.blobs(130, D, D)
    d = ref.extended_distances(X)
    eps_values, ms_values = ref.midpoint_eps(d), [1, 3, 5, 9]
    assert ref.relative_margin(d, eps_values) >= ref.MARGIN
    want = ref.cells_of_distances(d, [(e, m) for e in eps_values for m in ms_values])
    assert len({r["n_clusters"] for r in want}) >= 4 and any(r["n_border"] for r in want)
    same(learning.dbscan_sweep(X, eps_values, ms_values), want)


# ---- 7. rows holding infinities, through the C entry --------------------------------------------------------------------------
def test_rows_holding_infinities_are_nobodys_neighbours():
    """phk_dbscan_sweep_create refuses NaN only.  A distance to a row with an infinity is +inf or NaN and never <= eps: such
    a row is not even its own neighbour, so it is noise at min_samples = 1 too.  The restatement decides; the single-cell
    entry has to say the same."""
    from phamers_amd import _lib
    X, where = ref.rows_with_infinities()
    assert len(where) == 7 and not np.isnan(X).any() and not np.isfinite(X[where]).all(axis=1).any()
    cells = [(0.8, 4), (0.4, 1), (0.8, 1), (0.4, 4), (1e300, 1), (0.4, 108)]
    with np.errstate(invalid="ignore"):
        want = [ref.dbscan_sweep(X, [e], [m])[0] for e, m in cells]
    assert all((r["labels"][where] == -1).all() for r in want) and want[4]["n_core"] == 100 and want[4]["n_clusters"] == 1
    assert len({r["n_clusters"] for r in want}) >= 4
    ctx = _lib.get_context()
    rows = _lib.DbscanRows(ctx, X)
    try:
        got = ref.records_of_run(rows.run([e for e, _ in cells], [m for _, m in cells]), cells)
    finally:
        rows.close()
    same(got, want)
    for (eps, m), record in zip(cells, want):
        labels, core, k = _lib.dbscan(ctx, X, eps, m)
        assert np.array_equal(labels, record["labels"]) and np.array_equal(np.flatnonzero(core), record["core_sample_indices"])
        assert k == record["n_clusters"]
