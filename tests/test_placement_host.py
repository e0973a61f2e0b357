"""Host side of the per-contig placement and taxonomy prediction (no GPU): the enrichment test against the golden SciPy
values, the centring identity the device relies on, the lineage / label file readers, argument errors."""
import math

import numpy as np
import pytest

from oracle import oracle
from tests import helpers


@pytest.fixture(scope="module")
def doc():
    return helpers.load_json("placement.json")


@pytest.fixture(scope="module")
def probe():
    ref = helpers.load_npz("ref_features.npz")
    pos = oracle.normalize_counts(ref["pos_counts"].astype(np.int64))
    neg = oracle.normalize_counts(ref["neg_counts"].astype(np.int64))
    g = helpers.load_npz("placement.npz")
    contigs = np.vstack((neg[g["neg_rows"]], g["uniform_rows"], pos[g["dup_rows"]]))
    return pos, contigs, g


def test_find_enriched_classification_matches_the_reference(doc, probe):
    from phamers_amd import taxonomy
    pos, contigs, g = probe
    lineages = doc["lineages"]
    enriched = 0
    for case in doc["enrichment"]:
        b = doc["ids"].index(case["id"])
        a = g["assignments"][b]
        cluster_lineages = np.array([lineages[i] for i in np.flatnonzero(a[:-1] == a[-1])])
        kind, res, ratio = taxonomy.find_enriched_classification(cluster_lineages, lineages, case["depth"])
        assert kind == case["kind"], case
        if kind is None:
            assert res is None and ratio is None
            continue
        enriched += 1
        assert ratio == case["ratio"]
        print(case["id"], case["depth"], "chi2", res[0], case["chi2"], "p", res[1], case["p"])
        assert abs(res[0] - case["chi2"]) <= 1e-12 * abs(case["chi2"])
        assert abs(res[1] - case["p"]) <= 1e-12 * abs(case["p"])
        assert res[2] == case["dof"] == 1
        assert np.allclose(res[3], case["expected"], rtol=1e-14, atol=0)
    assert enriched >= 5 and enriched < len(doc["enrichment"])


def test_find_enriched_classification_degenerate_tables():
    from phamers_amd import taxonomy
    base = [["V", "a"]] * 6 + [["V", "b"]] * 6
    none = (None, None, None)
    assert taxonomy.find_enriched_classification([], base, 1) == none                    # empty cluster
    assert taxonomy.find_enriched_classification(base[:3], base, 0) == none              # x[1, 0] == 0: the whole base set
    assert taxonomy.find_enriched_classification([["V", "a"], ["V", "b"], ["V", "c"]], base, 1) == none   # ratio < 0.5
    assert taxonomy.find_enriched_classification(base, base, 1) == none                  # ratio 0.5 <= base ratio 0.5
    big = [["V", "a"]] * 10 + [["V", "b"]] * 190
    kind, res, ratio = taxonomy.find_enriched_classification([["V", "a"]] * 9 + [["V", "b"]], big, 1)
    assert kind == "a" and ratio == 0.9 and res[2] == 1 and res[1] < 1e-10


def test_chi2_p_value_is_the_one_degree_survival_function():
    from phamers_amd import taxonomy
    chi2, p, dof, expected = taxonomy.chi2_contingency_2x2([[12, 5], [7, 9]])
    # by hand: expected = row x column / total; Yates: |o - e| - 0.5
    e = np.outer([17, 16], [19, 14]) / 33.0
    want = (((np.abs(np.array([[12, 5], [7, 9]]) - e) - 0.5) ** 2) / e).sum()
    assert abs(chi2 - want) <= 1e-14 * want and dof == 1 and np.array_equal(expected, e)
    assert p == math.erfc(math.sqrt(chi2 / 2.0))


def test_centring_identity_bit_for_bit(probe):
    """NumPy's column mean of the appended matrix is (S + z) / (n + 1), S = the row-order column sum of the reference rows."""
    pos, contigs, _ = probe
    S = np.zeros(pos.shape[1])
    for row in pos:
        S = S + row
    assert np.array_equal(S, pos.sum(axis=0))
    for z in contigs:
        assert np.array_equal((S + z) / (pos.shape[0] + 1), np.vstack((pos, z[None, :])).mean(axis=0))


def test_lineage_and_label_file_readers(tmp_path):
    from phamers_amd import fileIO, taxonomy
    path = tmp_path / "lineages.txt"
    path.write_text("# id\tlineage\nNC_1\tViruses; dsDNA viruses; Caudovirales\nNC_2\tViruses;ssDNA viruses\nNC_3\tViruses\n")
    d = fileIO.read_label_file(str(path))
    assert d == {"NC_1": ["Viruses", "dsDNA viruses", "Caudovirales"], "NC_2": ["Viruses", "ssDNA viruses"], "NC_3": ["Viruses"]}
    assert fileIO.read_lineage_file(str(path)) == d
    e = fileIO.read_lineage_file(str(path), extend=True)
    assert [list(e[k]) for k in ("NC_1", "NC_2", "NC_3")] == [["Viruses", "dsDNA viruses", "Caudovirales"],
                                                             ["Viruses", "ssDNA viruses", "ssDNA viruses"],
                                                             ["Viruses", "Viruses", "Viruses"]]
    assert taxonomy.deepest_classification(d.values()) == 3
    with pytest.raises(TypeError):
        fileIO.read_label_file(None)


def test_place_contigs_argument_errors_need_no_device(monkeypatch):
    from phamers_amd import learning
    X = np.random.RandomState(0).rand(20, 8)
    assert learning.place_contigs(X, np.empty((0, 8)), 3) == []
    with pytest.raises(ValueError, match="NaN"):
        learning.place_contigs(X, np.full((1, 8), np.nan), 3)
    with pytest.raises(ValueError, match="infinity"):
        learning.place_contigs(X, np.full((1, 8), np.inf), 3)
    with pytest.raises(ValueError, match="dimension 1"):
        learning.place_contigs(X, np.zeros((2, 7)), 3)
    with pytest.raises(ValueError, match="n_clusters=22"):
        learning.place_contigs(X, np.zeros((1, 8)), 22)
    monkeypatch.setenv("PHAMERS_KMEANS", "gpu")
    with pytest.raises(NotImplementedError):
        learning.place_contigs(X, np.zeros((1, 8)), 3)


def test_placement_draws_are_those_of_the_seeding():
    """The draws handed to the device are the ones kmeans_plusplus_seeds consumes: same RandomState afterwards."""
    from phamers_amd import learning
    X = np.random.RandomState(1).rand(50, 6)
    rs = np.random.RandomState(learning.kmeans_seed)
    _, idx = learning.kmeans_plusplus_seeds(X, 7, rs)
    first, draws = learning.placement_draws(50, 7)
    assert first == idx[0] and draws.shape == (6, 2 + int(np.log(7)))
    rs2 = np.random.RandomState(learning.kmeans_seed)
    rs2.choice(50, p=np.ones(50) / 50)
    for row in draws:
        assert np.array_equal(row, rs2.uniform(size=draws.shape[1]))
    assert rs.uniform() == rs2.uniform()
