"""CPU-only: the host half of the likelihood-ranked lookup (phamers_amd/hosts.py) -- the Markov log
table, the argument rules that come before any device work, the p-value, the writer of phamer_hosts.csv and the parser --
and the restatement the GPU tests use (tests/hosts_ref.py)."""
import argparse

import numpy as np
import pytest

from tests import helpers, hosts_ref as ref


@pytest.fixture(scope="module")
def golden():
    g = helpers.load_npz("ref_features.npz")
    return g["pos_counts"].astype(np.int64), g["neg_counts"].astype(np.int64)


@pytest.fixture
def no_device(monkeypatch):
    from phamers_amd import _lib

    def refuse():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(_lib, "get_context", refuse)


def test_markov_table_against_the_logarithm_in_longdouble(golden):
    from phamers_amd import hosts
    neg = golden[1][:200]
    got = hosts.markov_log_table(neg)
    want = ref.markov_log_table(neg, dtype=np.longdouble)
    assert got.shape == (200, 256) and got.dtype == np.float64
    # one rounding each for the sum (exact: integers + a half), the quotient and the logarithm, on |log p| + 1
    assert (np.abs(got.astype(np.longdouble) - want) <= 4 * ref.U * (1 + np.abs(want))).all()
    assert np.array_equal(got, ref.markov_log_table(neg))
    other = hosts.markov_log_table(neg, pseudocount=0.01)
    assert (other != got).any() and np.isfinite(other).all()


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_every_prefix_group_sums_to_one(k):
    from phamers_amd import hosts
    rng = np.random.default_rng(k)
    x = rng.integers(0, 40, (7, 4 ** k))
    x[0] = 0                                        # no counts: every transition 1/4
    L = hosts.markov_log_table(x)
    sums = np.exp(L).reshape(7, 4 ** (k - 1), 4).sum(axis=2)
    assert np.abs(sums - 1.0).max() < 8 * ref.U
    assert np.array_equal(L[0], np.full(4 ** k, np.log(0.25)))
    # column 4 p + b: the k-mer with prefix p and last base b (first base = most significant digit)
    p = 4 ** (k - 1) - 1
    assert L[1, 4 * p + 2] == np.log((x[1, 4 * p + 2] + 0.5) / (x[1, 4 * p:4 * p + 4].sum() + 2.0))


def test_at_one_mers_the_markov_table_is_the_multinomial_table():
    from phamers_amd import hosts, likelihood
    x = np.random.default_rng(0).integers(0, 1000, (9, 4))
    assert np.array_equal(hosts.markov_log_table(x), likelihood.log_table(x))
    assert np.array_equal(hosts.markov_log_table(x, 0.1), likelihood.log_table(x, 0.1))


def test_argument_rules_come_before_device_work(no_device):
    from phamers_amd import _lib, hosts
    q, x = np.ones((3, 16), dtype=np.int64), np.arange(20 * 16).reshape(20, 16)
    assert _lib.HOSTS_MAX_TOP == 16
    for top in (0, 17, -1):
        with pytest.raises(ValueError, match="not in 1..16"):
            hosts.rank(q, x, top=top)
    with pytest.raises(ValueError, match="exceeds the 5 reference rows"):
        hosts.rank(q, x[:5], top=6)
    for bad in (np.ones((3, 8)), np.ones((3, 32)), np.ones((3, 1))):          # not 4^k columns
        with pytest.raises(ValueError, match="4\\^k columns"):
            hosts.markov_log_table(bad)
    with pytest.raises(ValueError, match="4\\^k columns"):
        hosts.rank(np.ones((3, 8)), np.ones((4, 8)), top=1, model='markov')
    with pytest.raises(ValueError, match="not frequencies"):
        hosts.rank(q / 16.0, x, top=1)
    with pytest.raises(ValueError, match="not frequencies"):
        hosts.markov_log_table(x / 7.0)
    with pytest.raises(ValueError, match="not frequencies"):
        hosts.fit_null(q / 16.0, x)
    with pytest.raises(ValueError, match="pseudocount"):
        hosts.rank(q, x, top=1, pseudocount=0.0)
    with pytest.raises(ValueError, match="model must be"):
        hosts.rank(q, x, top=1, model='euclid')
    with pytest.raises(ValueError, match="same number of columns"):
        hosts.rank(q[:, :4], x, top=1)
    # groups: a query must have `top` rows left
    rg = np.array([0] * 16 + [1, 1, -1, -1])
    with pytest.raises(ValueError, match="top = 5 exceeds the 4 reference rows query 1 \\(group 0\\) has left"):
        hosts.rank(q, x, top=5, query_groups=[1, 0, -1], reference_groups=rg)
    with pytest.raises(ValueError, match="one group id per row"):
        hosts.rank(q, x, top=1, query_groups=[1, 0], reference_groups=rg)
    with pytest.raises(ValueError, match="one entry per reference row"):
        hosts.rank(q, x, top=1, null=(np.zeros(3), np.ones(3)))
    # the null: at least two rows, every one with counts
    with pytest.raises(ValueError, match="at least 2 null rows"):
        hosts.fit_null(q[:1], x)
    with pytest.raises(ValueError, match="null row 1 has no counts"):
        hosts.fit_null(np.array([[1] * 16, [0] * 16, [2] * 16]), x)


def test_rows_left_counts_groups_from_the_histogram():
    from phamers_amd import hosts
    rg = np.array([3, 3, 7, -1, 7, 7], dtype=np.int32)
    hosts._check_rows_left(3, 6, np.array([7, 3, -1, 5], dtype=np.int32), rg)          # 3, 4, 6 and 6 rows left
    with pytest.raises(ValueError, match="query 0 \\(group 7\\)"):
        hosts._check_rows_left(4, 6, np.array([7, 3, -1, 5], dtype=np.int32), rg)
    hosts._check_rows_left(6, 6, np.array([7, 3], dtype=np.int32), None)               # groups on one side exclude nothing


def test_p_value():
    from phamers_amd import hosts
    import math
    z = np.array([[0.0, 1.0, -1.0], [np.nan, 8.0, -40.0]])
    p = hosts.p_value(z)
    assert p[0, 0] == 0.5 and p.shape == z.shape and np.isnan(p[1, 0]) and p[1, 2] == 1.0
    assert p[0, 1] == 0.5 * math.erfc(1.0 / math.sqrt(2.0)) and abs(p[0, 1] + p[0, 2] - 1.0) < 4 * ref.U
    assert 0.0 < p[1, 1] < 1e-14


def test_annotation_is_the_host_formula():
    from phamers_amd import hosts
    idx = np.array([[2, 0], [1, 2], [0, 1]])
    S = np.array([[-10.0, -12.0], [-3.0, -3.5], [0.0, 0.0]])
    totals = np.array([5, 2, 0], dtype=np.uint64)
    plain = hosts._annotate(idx, S, totals, None)
    assert plain.z is None and plain.p_value is None and plain.indices is idx and plain.log_likelihood is S
    assert np.array_equal(plain.per_kmer[:2], S[:2] / np.array([[5.0], [2.0]])) and np.isnan(plain.per_kmer[2]).all()
    mu, sigma = np.array([-2.0, -1.5, -2.5]), np.array([0.5, 0.25, 1.0])
    r = hosts._annotate(idx, S, totals, (mu, sigma))
    z, p = ref.z_and_p(plain.per_kmer, idx, mu, sigma)
    assert np.array_equal(r.z, z, equal_nan=True) and np.array_equal(r.p_value, p, equal_nan=True)
    assert r.z[0, 0] == (-2.0 - -2.5) / 1.0 and np.isnan(r.z[2]).all()


def test_restatement_ranks_by_likelihood_then_index():
    S = np.array([[1.0, 3.0, 3.0, -np.inf, 2.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    idx, val = ref.ranking(S, 3)
    assert idx.tolist() == [[1, 2, 4], [0, 1, 2]] and val[0].tolist() == [3.0, 3.0, 2.0]
    out = ref.excluded([0, -1], [0, 1, 0, -1, -1], 2, 5)
    assert out.tolist() == [[True, False, True, False, False], [False] * 5]
    idx, _ = ref.ranking(S, 2, out)
    assert idx.tolist() == [[1, 4], [0, 1]]
    # check_ranking accepts the statement's own float64 ranking and refuses a swapped one
    rng = np.random.default_rng(4)
    c, x = rng.integers(0, 30, (6, 16)), rng.integers(1, 90, (12, 16))
    L = ref.table(x, 'markov')
    S_ld, e = ref.products(c, L), ref.bound(c, L)
    idx, val = ref.ranking(ref.products(c, L, np.float64), 4)
    assert ref.check_ranking(idx, val, S_ld, e, 4) == 1.0
    with pytest.raises(AssertionError):
        ref.check_ranking(idx[:, ::-1].copy(), val[:, ::-1].copy(), S_ld, e, 4)


def test_null_restatement_in_float64_is_within_its_own_bound(golden):
    pos, neg = golden
    L = ref.table(neg[:40], 'markov')
    mu, sigma, _ = ref.null_statement(pos[:300], L, np.float64)
    t_mu, t_sigma = ref.check_null(mu, sigma, pos[:300], L, what="float64 statement")
    assert (t_mu < 1e-11).all() and (t_sigma < 1e-10).all() and (sigma > 1e-3).all()      # the bound means something
    assert np.allclose(mu, (pos[:300] @ L.T / pos[:300].sum(axis=1)[:, None]).mean(axis=0), rtol=1e-12)
    assert np.allclose(sigma, (pos[:300] @ L.T / pos[:300].sum(axis=1)[:, None]).std(axis=0, ddof=1), rtol=1e-10)


def test_parser_and_refusals(no_device):
    from phamers_amd import phamer
    ap = phamer._parser()
    plain = ap.parse_args(["-in", "x"])
    assert not hasattr(plain, "hosts") and not hasattr(plain, "hosts_model")      # the stamped summary stays as it was
    given = ap.parse_args(["-in", "x", "--hosts", "3", "--hosts_model", "multinomial"])
    assert given.hosts == 3 and given.hosts_model == "multinomial"
    assert not hasattr(ap.parse_args(["-in", "x", "--hosts", "3"]), "hosts_model")
    for argv in (["-in", "x", "--hosts", "3", "--gpus", "2"], ["-in", "x", "--hosts", "0"], ["-in", "x", "--hosts", "17"],
                 ["-in", "x", "--hosts_model", "markov"], ["-in", "x", "--hosts", "2", "--hosts_model", "euclid"]):
        with pytest.raises(SystemExit) as e:
            phamer.main(argv)
        assert e.value.code == 2


def test_scorer_needs_count_rows(no_device):
    from phamers_amd import phamer
    sc = phamer.phamer_scorer()
    assert sc.keep_reference_counts is False
    sc.positive_data, sc.negative_data = np.full((3, 4), 0.25), np.full((3, 4), 0.25)
    with pytest.raises(ValueError, match="needs the reference COUNT rows"):
        sc.predict_hosts(2)
    sc.positive_counts, sc.negative_counts = np.ones((3, 4), dtype=np.int64), np.ones((3, 4), dtype=np.int64)
    with pytest.raises(ValueError, match="integer k-mer counts"):
        sc.predict_hosts(2)


def test_hosts_file_round_trips(tmp_path):
    from phamers_amd import fileIO, phamer
    sc = phamer.phamer_scorer()
    sc.output_directory = str(tmp_path)
    assert sc.get_hosts_output_filename() == str(tmp_path / "phamer_hosts.csv")
    sc.data_ids = np.array(["c,1", "c2"], dtype=object)
    sc.host_ids = np.array([["NC_1", "NC_2"], ["NC_3", "NC_1"]], dtype=object)
    sc.host_log_likelihood = np.array([[-6543.25, -6600.0], [0.0, 0.0]])
    sc.host_per_kmer = np.array([[-1.3, -1.32], [np.nan, np.nan]])
    sc.host_z = np.array([[2.5, 0.1 + 0.2], [np.nan, np.nan]])
    sc.host_p_value = np.array([[0.006, 0.4], [np.nan, np.nan]])
    sc.make_hosts_file(args=argparse.Namespace(hosts=2, input_directory="in"))
    lines = open(sc.get_hosts_output_filename()).read().split("\n")
    assert lines[0] == "# PhaMers host prediction file" and "# hosts:\t2" in lines
    body = [ln for ln in lines if not ln.startswith("#")]
    assert body[0] == "contig_id,rank,host_id,log_likelihood,per_kmer,z,p_value"
    assert body[1] == '"c,1",1,NC_1,-6543.25,-1.3,2.5,0.006' and body[2] == '"c,1",2,NC_2,-6600.0,-1.32,%r,0.4' % (0.1 + 0.2)
    assert body[3] == "c2,1,NC_3,0.0,nan,nan,nan" and body[5:] == [""]
    rows = fileIO.read_phamer_hosts(sc.get_hosts_output_filename())
    assert rows[0] == ("c,1", 1, "NC_1", -6543.25, -1.3, 2.5, 0.006) and rows[2][:4] == ("c2", 1, "NC_3", 0.0)
    with pytest.raises(ValueError, match="hits"):
        fileIO.save_phamer_hosts(str(tmp_path / "bad.csv"), sc.data_ids[:1], sc.host_ids, sc.host_log_likelihood,
                                 sc.host_per_kmer, sc.host_z, sc.host_p_value)


def test_the_first_batch_s_groups_in_every_batch_return_rows_of_the_query_s_group():
    """The inputs of test_groups_across_batches_do_not_change_a_bit (tests/test_gpu_hosts.py): had batches 2 and 3 read batch
    1's group ids, at least half of their queries would get another list than the statement's -- by more than the bound: a row
    of the query's own group comes back, or a row is missing whose S exceeds the last returned one's by more than 2 e.  So
    that test can fail."""
    from tests import test_gpu_hosts as gpu
    rng = np.random.default_rng(21)                                      # the GPU tests' ``shapes`` fixture
    q, x = gpu._contigs(rng, 300, 256), gpu._genomes(rng, 513, 256)
    gq, gr = ref.random_groups(4, 300), ref.random_groups(5, 513)
    wrong = ref.groups_of_the_first_batch(gq)
    assert np.array_equal(wrong[:128], gq[:128]) and (wrong[128:] != gq[128:]).mean() > 0.5
    out = ref.excluded(gq, gr, 300, 513)
    assert (~out).sum(axis=1).min() >= 16
    for model in gpu.MODELS:
        L = ref.table(x, model)
        S, e = ref.products(q, L), ref.bound(q, L)
        for top in (5, 16):
            right, _ = ref.ranking(S, top, out)
            mistaken, _ = ref.ranking(S, top, ref.excluded(wrong, gr, 300, 513))
            assert np.array_equal(mistaken[:128], right[:128])
            caught = np.zeros(300, dtype=bool)
            for i in range(128, 300):
                own = out[i, mistaken[i]].any()
                rest = ~out[i]
                rest[mistaken[i]] = False
                caught[i] = own or float(S[i, rest].max() - S[i, mistaken[i, -1]]) > 2.0 * e[i]
            assert caught[128:].mean() >= 0.5, (model, top, caught[128:].mean())
