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
