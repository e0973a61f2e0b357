"""CPU-only: the host restatement of the nearest-reference lookup against NumPy on the golden queries, the argument checks
that come before any device work, and the writer of phamer_neighbors.csv."""
import argparse

import numpy as np
import pytest

from tests import helpers, neighbors_ref as ref


@pytest.fixture(scope="module")
def golden():
    X, ids, n_pos = ref.reference_rows(helpers.GOLDEN)
    return helpers.load_npz("scoring_k4.npz")["q"], X


def test_restatement_against_numpy_on_the_golden_queries(golden):
    """Both sides sum D squares of rounded differences in float64: each is within (D + 2) 2^-53 of the true squared
    distance relatively, the roots within half of that plus a rounding -- 4 (D + 2) 2^-53 between them covers it."""
    Q, X = golden
    D, k = Q.shape[1], 5
    tol = 4 * (D + 2) * 2.0 ** -53
    dist, idx = ref.kneighbors_screened(Q, X, k)
    for a in range(Q.shape[0]):
        d = np.linalg.norm(X - Q[a], axis=1)
        order = np.argsort(d, kind="stable")[:k + 1]
        want = d[order[:k]]
        assert np.all(np.abs(dist[a] - want) <= tol * want), a
        clear = np.diff(d[order]) > 2 * tol * d[order[1:]]           # the neighbour and the next one are told apart
        sure = np.concatenate(([True], clear[:-1])) & clear           # ... on both sides of a position
        assert np.array_equal(idx[a][sure], order[:k][sure]), a


def test_screened_restatement_is_the_full_chain(golden):
    Q, X = golden
    for k in (1, 5, 28):
        d_full, i_full = ref.kneighbors_ref(Q[:4], X, k)
        d_scr, i_scr = ref.kneighbors_screened(Q[:4], X, k)
        assert np.array_equal(i_full, i_scr) and np.array_equal(d_full.view(np.int64), d_scr.view(np.int64))


def test_restatement_orders_ties_by_index_and_honours_the_mask():
    X = np.array([[0.0, 1.0], [1.0, 0.0], [0.0, 1.0], [0.0, -1.0], [3.0, 0.0]])
    dist, idx = ref.kneighbors_ref(np.zeros((1, 2)), X, 4)
    assert idx.tolist() == [[0, 1, 2, 3]] and dist.tolist() == [[1.0, 1.0, 1.0, 1.0]]
    dist, idx = ref.kneighbors_ref(np.zeros((1, 2)), X, 4, mask=[False, True, False, False, False])
    assert idx.tolist() == [[0, 2, 3, 4]] and dist.tolist() == [[1.0, 1.0, 1.0, 3.0]]


@pytest.mark.parametrize("k, queries, data", [
    (0, np.zeros((3, 4)), np.ones((40, 4))),
    (29, np.zeros((3, 4)), np.ones((40, 4))),
    (7, np.zeros((3, 4)), np.ones((6, 4))),          # k > M
    (2, np.zeros(4), np.ones((40, 4))),              # not 2-D
    (2, np.zeros((3, 4)), np.ones((2, 20, 4))),
    (2, np.zeros((3, 5)), np.ones((40, 4))),         # width mismatch
])
def test_bad_arguments_are_refused_before_device_work(monkeypatch, k, queries, data):
    from phamers_amd import _lib, learning

    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(_lib, "get_context", no_device)
    with pytest.raises(ValueError):
        learning.kneighbors(queries, data, k=k)


def test_command_line_flag(monkeypatch):
    from phamers_amd import _lib, phamer
    monkeypatch.setattr(_lib, "get_context", lambda: pytest.fail("the device was asked for"))
    ap = phamer._parser()
    assert ap.parse_args(["-in", "x", "--neighbors", "3"]).neighbors == 3
    assert not hasattr(ap.parse_args(["-in", "x"]), "neighbors")        # the stamped argument summary stays as it was
    assert ap.parse_args(["-in", "x", "-n", "neg.fasta"]).negative_fasta == "neg.fasta"
    for argv in (["-in", "x", "--neighbors", "3", "--gpus", "2"], ["-in", "x", "--neighbors", "0"],
                 ["-in", "x", "--neighbors", "29"]):
        with pytest.raises(SystemExit) as e:
            phamer.main(argv)
        assert e.value.code == 2


def test_neighbors_file_round_trips(tmp_path):
    from phamers_amd import fileIO, phamer
    scorer = phamer.phamer_scorer()
    scorer.output_directory = str(tmp_path)
    assert scorer.get_neighbors_output_filename() == str(tmp_path / "phamer_neighbors.csv")
    scorer.data_ids = np.array(["contig,with,commas", 'quoted "id"', "plain_3"])
    scorer.positive_data, scorer.negative_data = np.zeros((2, 4)), np.zeros((3, 4))
    scorer.positive_ids, scorer.negative_ids = np.array(["P0", "P,1"]), np.array(["N0", "N1", "N 2"])
    scorer.neighbor_indices = np.array([[1, 4], [0, 2], [3, 1]])
    scorer.neighbor_distances = np.array([[0.0, 0.1], [1e-300, 2.0 / 3.0], [5e-324, 1.7976931348623157e308]])
    scorer.neighbor_ids = np.concatenate((scorer.positive_ids, scorer.negative_ids))[scorer.neighbor_indices]
    scorer.make_neighbors_file(args=argparse.Namespace(neighbors=2, input_directory="in,dir"))
    text = open(scorer.get_neighbors_output_filename()).read()
    lines = text.split("\n")
    assert lines[0] == "# PhaMers nearest reference file" and "# neighbors:\t2" in lines
    body = [ln for ln in lines if ln and not ln.startswith("#")]
    assert body[0] == "contig_id,rank,reference_id,class,distance" and len(body) == 7
    assert body[2].endswith(",2,N 2,negative,0.1")                     # repr(float), not a fixed format
    rows = fileIO.read_phamer_neighbors(scorer.get_neighbors_output_filename())
    want = [(scorer.data_ids[a], r + 1, scorer.neighbor_ids[a][r], "positive" if scorer.neighbor_indices[a][r] < 2 else "negative",
             scorer.neighbor_distances[a][r]) for a in range(3) for r in range(2)]
    assert rows == [(str(c), r, str(i), kind, float(d)) for c, r, i, kind, d in want]
    assert [repr(r[4]) for r in rows] == [ln.rsplit(",", 1)[1] for ln in body[1:]]


# ---- the helpers of tests/test_gpu_neighbors_shapes.py -------------------------------------------------------------------
def test_lattice_sqdist_is_the_chain_and_refuses_other_input():
    rng = np.random.default_rng(21)
    X = rng.integers(0, 16, (700, 2)) * 2.0 ** -6
    Q = rng.integers(0, 32, (40, 2)) * 2.0 ** -7
    assert ref.lattice_unit(Q, X) == 2.0 ** -7 and ref.lattice_unit(np.zeros((2, 2))) == 1.0
    assert ref.lattice_unit(np.array([[3.0, -0.75]]), np.array([[2.0 ** 60]])) == 0.25
    got = ref.lattice_sqdist(Q, X)
    assert np.array_equal(got.view(np.int64), ref.sqdist(Q, X).view(np.int64))
    X16 = rng.integers(64, 192, (50, 16)) * 2.0 ** -8                     # the lattice of the ties tests
    assert np.array_equal(ref.lattice_sqdist(X16[:7], X16).view(np.int64), ref.sqdist(X16[:7], X16).view(np.int64))
    for s in (2.0 ** 200, 2.0 ** -200):                                    # a power of two moves the unit, nothing else
        assert np.array_equal(ref.lattice_sqdist(Q * s, X * s), got * (s * s))
    with pytest.raises(AssertionError, match="lattice"):
        ref.lattice_sqdist(rng.random((3, 2)), X)                          # off the lattice: a unit of 2^-53 or so
    with pytest.raises(AssertionError, match="lattice"):
        ref.lattice_sqdist(Q + 2.0 ** -40, X)
    with pytest.raises(AssertionError, match="lattice"):                   # on a lattice, but the sums pass 2^53
        ref.lattice_sqdist(np.array([[2.0 ** 27, 0.0]]), np.array([[-1.0, 1.0]]))
    ref.lattice_sqdist(np.array([[2.0 ** 25, 0.0]]), np.array([[-1.0, 1.0]]))


def test_select_by_partition_is_select():
    rng = np.random.default_rng(22)
    d2 = rng.integers(0, 6, (30, 200)).astype(np.float64)                 # long tie classes
    d2[:, 7] = np.inf
    for k in (1, 4, 28):
        a, b = ref.select(d2, k), ref.select_by_partition(d2, k)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.int64), b[0].view(np.int64))


def test_route_predicates_on_a_hand_made_tie_class():
    """One query, values 0, 1, 1, 1, then c rows at 2, then 10, 11, ...: the class at 2 holds places 5 .. 4 + c."""
    E = np.array([0.01])

    def row(c, m=60):
        return np.concatenate(([0.0, 1.0, 1.0, 1.0], np.full(c, 2.0), 10.0 + np.arange(m - 4 - c)))[None, :]
    # k = 5 (KC = 16): place 5 is in the class.  It must fall back as soon as the class passes the list ...
    assert not ref.must_fall_back(row(12), 5, 16)[0] and ref.must_fall_back(row(13), 5, 16)[0]
    # ... and must be certified only while place KC = 16 lies beyond the class: at c = 12 place 16 is the class's last
    # row, the gap is 0 and nothing is claimed (the class can fill the list and a~_(16) - E fall below d2_(5))
    assert ref.must_certify(row(11), E, 5, 16)[0] and not ref.must_certify(row(12), E, 5, 16)[0]
    assert not ref.must_certify(row(13), E, 5, 16)[0]
    # k = 4 (KC = 8): place 4 is in the class of three at 1 with 0 before it -- certified by the gap to place 8 ...
    assert ref.must_certify(row(2), E, 4, 8)[0] and not ref.must_fall_back(row(2), 4, 8)[0]
    assert ref.must_certify(row(5), E, 4, 8)[0]                           # place 8 is 2.0: a gap of 1 against 4 E = 0.04
    # ... and the bound decides: the same rows, gaps of 8 and of 1 against 4 E (strictly greater)
    assert not ref.must_certify(row(5), np.array([0.25]), 4, 8)[0] and ref.must_certify(row(5), np.array([0.2]), 4, 8)[0]
    assert ref.must_certify(row(11), np.array([0.2]), 5, 16)[0] and not ref.must_certify(row(11), np.array([2.0]), 5, 16)[0]
    # masked rows are +inf: with at most KC finite rows every row is kept, whatever the ties
    few = np.full((1, 60), np.inf)
    few[0, [3, 30, 31, 59]] = 2.0
    few[0, [4, 5, 6, 7]] = 3.0
    assert ref.must_certify(few, E, 4, 8)[0] and not ref.must_fall_back(few, 4, 8)[0]
    few[0, 40] = 2.0                                                       # nine finite rows, five of them at place 4:
    assert ref.must_certify(few, E, 4, 8)[0] and not ref.must_fall_back(few, 4, 8)[0]      # the list takes the class, 3.0 is beyond
    few[0, 41:44] = 2.0                                                    # eight rows at place 4 fill the list: no claim
    assert not ref.must_certify(few, E, 4, 8)[0] and not ref.must_fall_back(few, 4, 8)[0]
    few[0, 44] = 2.0                                                       # nine rows at place 4
    assert ref.must_fall_back(few, 4, 8)[0] and not ref.must_certify(few, E, 4, 8)[0]
    assert ref.must_certify(row(12, 16), E, 5, 16)[0]                      # M <= KC: every row kept, whatever the ties


@pytest.mark.parametrize("D", [24, 32])
def test_route_predicates_on_random_counts(D):
    """Rows of normalised counts are far apart in units of E: every query must be certified at every list length, none
    must fall back, and the two predicates never both hold."""
    rng = np.random.default_rng(23 + D)
    Q, X = ref.normalised_counts(rng, 40, D), ref.normalised_counts(rng, 300, D)
    d2 = ref.sqdist(Q, X)
    for M in (29, 33, 300):
        E = ref.bound_E(Q, X[:M])
        for k, KC in ((4, 8), (12, 16), (28, 32)):
            yes, no = ref.must_certify(d2[:, :M], E, k, KC), ref.must_fall_back(d2[:, :M], k, KC)
            assert yes.all() and not no.any()
            if M > KC:
                s = np.sort(d2[:, :M], axis=1)
                assert np.all((s[:, KC - 1] - s[:, k - 1]) > 1e6 * E)       # the margin the device tests rely on
    tied = d2.copy()
    tied[:, 100:140] = tied[:, [5]]                                       # 41 rows share a value
    for k, KC in ((4, 8), (28, 32)):
        yes, no = ref.must_certify(tied, ref.bound_E(Q, X), k, KC), ref.must_fall_back(tied, k, KC)
        assert not (yes & no).any()
        r5 = (tied < tied[:, [5]]).sum(axis=1)                            # rows strictly before the class
        assert np.array_equal(no, (r5 < k))                                # place k falls into the class of 41 > KC
