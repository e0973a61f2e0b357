"""GPU: the multinomial likelihood scoring method (likelihood.hip, phamers_amd/likelihood.py) against its extended
precision statement (tests/likelihood_ref.py) within the bound derived there, and bit equality across batch splits,
entry points, strands and runs.  Shapes are the smallest that cross the kernel's boundaries: the query block is 128, the
row chunk 256, a row step 64, a column step 32."""
import numpy as np
import pytest

from tests import helpers, likelihood_ref as ref

pytestmark = pytest.mark.gpu


def _contigs(rng, n, D, kmers=4997):
    """Count rows of n contigs of ``kmers`` k-mers each, every one from a profile of its own."""
    return np.stack([rng.multinomial(kmers, rng.dirichlet(np.full(D, 0.7))) for _ in range(n)]).astype(np.uint32)


def _genomes(rng, n, D):
    return np.stack([rng.multinomial(int(rng.integers(3000, 200000)), rng.dirichlet(np.full(D, 0.7))) for _ in range(n)])


@pytest.fixture(scope="module")
def golden():
    g = helpers.load_npz("ref_features.npz")
    return g["pos_counts"].astype(np.int64), g["neg_counts"].astype(np.int64)


@pytest.fixture(scope="module")
def shapes():
    """One set of random rows for all the D = 256 shape cases: 300 queries, 513 + 257 reference rows, cut as needed."""
    rng = np.random.default_rng(20)
    return _contigs(rng, 300, 256), _genomes(rng, 513, 256), _genomes(rng, 257, 256)


def _score_with_details(q, pos, neg, **kw):
    from phamers_amd import likelihood
    d = {}
    s = likelihood.score(q, pos, neg, _details=d, **kw)
    return d["l_pos"], d["l_neg"], s


# ---- 1. query and row shapes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 127, 128, 129])
@pytest.mark.parametrize("m_pos,m_neg", [(1, 1), (255, 257), (513, 16)])
def test_shapes_against_extended_statement(shapes, n, m_pos, m_neg):
    q, pos, neg = shapes
    q, pos, neg = q[:n], pos[:m_pos], neg[:m_neg]
    got = _score_with_details(q, pos, neg)
    assert all(v.shape == (n,) and v.dtype == np.float64 for v in got)
    ref.check(got, q, ref.log_table(pos), ref.log_table(neg), what="N=%d M=(%d, %d)" % (n, m_pos, m_neg))
    assert np.array_equal(got[2], got[0] - got[1])


def test_batch_splits_do_not_change_a_bit(shapes):
    q, pos, neg = shapes
    whole = _score_with_details(q, pos, neg)
    ref.check(whole, q, ref.log_table(pos), ref.log_table(neg), what="300 queries")
    split = _score_with_details(q, pos, neg, _batch_rows=128)          # three batches: 128 + 128 + 44
    small = _score_with_details(q, pos, neg, _batch_rows=1)            # rounded up to the query block
    for a, b, c in zip(whole, split, small):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    # nor does N, or where in the call a query stands
    for lo, hi in ((0, 1), (0, 129), (127, 300), (299, 300)):
        part = _score_with_details(q[lo:hi], pos, neg)
        assert all(np.array_equal(a[lo:hi], b) for a, b in zip(whole, part))
    again = _score_with_details(q, pos, neg)                            # run to run
    assert all(np.array_equal(a, b) for a, b in zip(whole, again))


@pytest.mark.parametrize("classes", [2, 1])
@helpers.timed
def test_groups_across_batches_do_not_change_a_bit(shapes, classes):
    """Random group ids on both sides and more than one device batch: each batch must read its own queries' ids and its own
    effective row counts.  (tests/test_likelihood_host.py: with the first batch's ids in every batch most queries leave the bound.)"""
    from phamers_amd import _lib
    q, pos, neg = shapes
    lp, ln = ref.log_table(pos), (ref.log_table(neg) if classes == 2 else None)
    gq, gp, gn = ref.random_groups(1, 300), ref.random_groups(2, 513), (ref.random_groups(3, 257) if classes == 2 else None)
    table = _lib.LikelihoodTable(_lib.get_context(), lp, ln, gp, gn)

    def score(rows, groups, batch_rows):
        d = {}
        s = table.score(rows, groups, batch_rows, d)
        return d["l_pos"], d["l_neg"], s

    try:
        whole = score(q, gq, 0)
        ref.check(whole, q, lp, ln, gq, gp, gn, what="groups, %d classes" % classes)
        for batch_rows in (128, 1):                                      # three batches: 128 + 128 + 44
            assert all(np.array_equal(a, b) for a, b in zip(whole, score(q, gq, batch_rows)))
        part = score(q[127:300], gq[127:300], 128)                       # the ids travel with their queries
        assert all(np.array_equal(a[127:300], b) for a, b in zip(whole, part))
        assert not np.array_equal(whole[2], score(q, None, 0)[2])        # and they exclude something
    finally:
        table.close()


# ---- 2. other D ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 16, 64, 1024])
def test_other_widths_through_a_resident_batch(D):
    """D = 4 and 16 are the widths a batch accepts that are no multiple of the column step: the guarded loader."""
    from phamers_amd import _lib, likelihood
    rng = np.random.default_rng(D)
    q, pos, neg = _contigs(rng, 131, D, kmers=2500), _genomes(rng, 70, D), _genomes(rng, 65, D)
    q[5] = 0
    lp, ln = likelihood.log_table(pos), likelihood.log_table(neg)
    ctx = _lib.get_context()
    table = _lib.LikelihoodTable(ctx, lp, ln)
    batch = _lib.Batch.from_counts(ctx, q)
    assert batch is not None and batch.D == D
    try:
        d = {}
        got = batch.likelihood(table, details=d)
        host = table.score(q)
    finally:
        batch.close()
        table.close()
    ref.check((d["l_pos"], d["l_neg"], got), q, lp, ln, what="D=%d" % D)
    assert np.array_equal(got, host) and np.array_equal(got, likelihood.score(q, pos, neg))
    assert got[5] == 0.0


# ---- 3. edge rows ----------------------------------------------------------------------------------------------------------
def test_edge_rows(golden):
    from phamers_amd import likelihood
    pos, neg = golden
    pos, neg = pos[:300], neg[:300]
    lp, ln = ref.log_table(pos), ref.log_table(neg)
    zero = np.zeros(256, dtype=np.int64)
    one = zero.copy()
    one[27] = 1
    homo = zero.copy()
    homo[0] = 4997
    q = np.stack((zero, one, homo))
    got = _score_with_details(q, pos, neg)
    ref.check(got, q, lp, ln, what="edge rows")
    assert got[0][0] == 0.0 and got[1][0] == 0.0 and got[2][0] == 0.0           # no counts: exactly 0
    per_kmer = likelihood.score(q, pos, neg, per_kmer=True)
    assert np.isnan(per_kmer[0]) and per_kmer[1] == got[2][1] and per_kmer[2] == got[2][2] / 4997.0
    # a homopolymer against profiles whose entry there came from the pseudocount alone
    bare_p, bare_n = pos.copy(), neg.copy()
    bare_p[:, 0], bare_n[:, 0] = 0, 0
    got = _score_with_details(q[2:], bare_p, bare_n)
    ref.check(got, q[2:], ref.log_table(bare_p), ref.log_table(bare_n), what="homopolymer, bare column")
    assert np.isfinite(got[2]).all() and got[0][0] < -4997 * 5


def test_longest_rows_need_the_max_subtraction(golden):
    """The 3.5M-k-mer bacterial rows against the phage rows: S ~ -2e7, where exp(S) is 0 and a plain log-sum-exp -inf."""
    pos, neg = golden
    big = neg[np.argsort(neg.sum(axis=1))[-8:]]
    pos, neg = pos[:300], neg[:300]
    lp, ln = ref.log_table(pos), ref.log_table(neg)
    assert big.sum(axis=1).min() > 3000000
    with np.errstate(divide='ignore'):
        assert np.isneginf(np.log(np.exp(big.astype(np.float64) @ lp.T).sum(axis=1))).all()
    got = _score_with_details(big, pos, neg)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and (got[0] < -1e7).all()
    ref.check(got, big, lp, ln, what="longest rows")


# ---- 4. the validator's folds on golden rows -------------------------------------------------------------------------------
@pytest.mark.parametrize("folds", [20, "loo"])
def test_cross_validation_on_golden_rows(golden, folds):
    from phamers_amd import cross_validate, learning, likelihood
    pos, neg = golden
    pos, neg = pos[:300], neg[:300]
    lp, ln = ref.log_table(pos), ref.log_table(neg)
    if folds == "loo":
        gp, gn = np.arange(300), 300 + np.arange(300)
    else:
        plan = cross_validate.FoldPlan(300, 300, folds, 0)
        gp, gn = plan.positive, plan.negative
    ps, ns = likelihood.cross_validate(pos, neg, folds, 0)
    q, qg = np.vstack((pos, neg)), np.concatenate((gp, gn))
    # each held-out row against the statement computed with its group's rows DELETED
    want = np.empty(600, dtype=np.longdouble)
    tol = np.empty(600)
    got = np.concatenate((ps, ns))
    for g in np.unique(qg):
        rows = qg == g
        w = ref.statement(q[rows], lp[gp != g], ln[gn != g], dtype=np.longdouble)
        want[rows], tol[rows] = w[2], ref.tolerance(q[rows], lp[gp != g], ln[gn != g], w[0], w[1])
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    assert (err <= tol).all(), (err / tol).max()
    # no positive and negative score within the bound of each other: the ranking, and so the integer area, is exact
    w64 = want.astype(np.float64)
    assert (np.abs(w64[:300, None] - w64[None, 300:]) > tol[:300, None] + tol[None, 300:] + 1e-9).all()
    auc = learning.predictor_performance(ps, ns)[2]
    assert auc == learning.predictor_performance(w64[:300], w64[300:])[2]
    assert abs(auc - (w64[:300, None] > w64[None, 300:]).sum() / 90000.0) < 1e-12
    assert auc > 0.98
    # the validator routes the method here, and its reports work on the scores
    v = cross_validate.cross_validator()
    v.method, v.N, v.seed = "likelihood", (300 if folds == "loo" else folds), 0
    v.positive_counts, v.negative_counts = pos, neg
    if folds != "loo":
        vp, vn = v.cross_validate()
        assert np.array_equal(vp, ps) and np.array_equal(vn, ns) and np.array_equal(v.positive_assignment, gp)
        assert v.performance()[2] == auc
    # per k-mer: the same scores over the rows' totals
    pk, nk = likelihood.cross_validate(pos, neg, folds, 0, per_kmer=True)
    assert np.array_equal(pk, ps / pos.sum(axis=1)) and np.array_equal(nk, ns / neg.sum(axis=1))


def test_command_line_writes_the_table(golden, tmp_path):
    from phamers_amd import fileIO, likelihood
    pos, neg = golden
    pos, neg = pos[:120], neg[:110]
    pf, nf, out = str(tmp_path / "p.csv"), str(tmp_path / "n.csv"), str(tmp_path / "table.csv")
    fileIO.save_counts(pos, ["p%d" % i for i in range(len(pos))], pf)
    fileIO.save_counts(neg, ["n%d" % i for i in range(len(neg))], nf)
    assert likelihood.main(["-pf", pf, "-nf", nf, "-N", "5", "--seed", "3", "--lengths", "200", "1000", "-out", out]) == 0
    lines = open(out).read().split("\n")
    assert lines[0] == "length,auc,accuracy" and [ln.split(",")[0] for ln in lines[1:4]] == ["full", "200", "1000"]
    assert lines[4:] == [""]
    full = likelihood.evaluate(*likelihood.cross_validate(pos, neg, 5, 3))
    assert lines[1] == "full,%r,%r" % (float(full[0]), float(full[1]))
    rng = np.random.RandomState(3)
    short = likelihood.thin(pos, 200, rng), likelihood.thin(neg, 200, rng)
    want = likelihood.evaluate(*likelihood.cross_validate(pos, neg, 5, 3, _queries=short))
    assert lines[2] == "200,%r,%r" % (float(want[0]), float(want[1]))
    assert float(lines[2].split(",")[1]) < float(lines[3].split(",")[1]) <= 1.0       # fewer k-mers, smaller area


def test_groups_and_one_class(shapes):
    from phamers_amd import _lib, likelihood
    q, pos, neg = shapes
    q, pos = q[:140], pos[:300]
    lp = ref.log_table(pos)
    one = likelihood.log_likelihood(q, pos)
    ref.check((one, np.zeros(140), one), q, lp, what="one class")
    gq, gr = np.arange(140) % 5 - 1, np.arange(300) % 7 - 1             # some without a group on both sides
    got = likelihood.log_likelihood(q, pos, query_groups=gq, reference_groups=gr)
    ref.check((got, np.zeros(140), got), q, lp, None, gq, gr, what="one class, groups")
    assert np.array_equal(got[gq < 0], one[gq < 0]) and not np.array_equal(got, one)
    assert np.array_equal(likelihood.log_likelihood(q, pos, query_groups=gq), one)       # groups on one side: none excluded
    with pytest.raises(ValueError, match="leaves no positive row"):
        likelihood.log_likelihood(q[:3], pos[:4], query_groups=[0, 2, 0], reference_groups=[2, 2, 2, 2])
    table = _lib.LikelihoodTable(_lib.get_context(), lp[:4], lp[:2], [0, 1, 2, 3], [5, 5])
    try:
        with pytest.raises(ValueError, match="leaves no negative row"):
            table.score(q[:2], [0, 5])
        with pytest.raises(ValueError, match="counts must be"):
            table.score(q[:2, :16])
    finally:
        table.close()
    bad = lp[:2].copy()
    bad[1, 3] = -np.inf
    with pytest.raises(ValueError, match="not finite"):
        _lib.LikelihoodTable(_lib.get_context(), bad)


# ---- 5. entry points ---------------------------------------------------------------------------------------------------------
def _write_inputs(tmp_path, seqs, pos, neg):
    from phamers_amd import fileIO
    data = tmp_path / "data" / "reference_features"
    data.mkdir(parents=True)
    fileIO.save_counts(pos, ["p%d" % i for i in range(len(pos))], str(data / "positive_features.csv"))
    fileIO.save_counts(neg, ["n%d" % i for i in range(len(neg))], str(data / "negative_features.csv"))
    indir = tmp_path / "in"
    indir.mkdir()
    with open(indir / "contigs.fasta", "w") as f:
        for c, s in enumerate(seqs):
            f.write(">SuperContig_%d_length_%d_ID_%d\n" % (c, len(s), c))
            f.write("\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + "\n")
    return indir, tmp_path / "data"


def _scorer(indir, data, **attrs):
    from phamers_amd import phamer
    sc = phamer.phamer_scorer()
    sc.scoring_method = "likelihood"
    for k, v in attrs.items():
        setattr(sc, k, v)
    sc.input_directory, sc.data_directory = str(indir), str(data)
    sc.find_data_files()
    sc.load_data()
    try:
        return sc, sc.score_points()
    finally:
        sc._drop_batch()


def test_entry_points_agree_bit_for_bit(golden, tmp_path):
    from phamers_amd import _lib, likelihood, synth, transform_kmers
    from tests import strands_ref
    pos, neg = golden
    pos, neg = pos[:150], neg[:140]
    seqs = [synth.synth_contig(11, c, 5000 + 37 * c) for c in range(20)]
    ctx = _lib.get_context()
    counted = _lib.Batch.from_sequences(ctx, seqs, 4)
    table = _lib.LikelihoodTable(ctx, likelihood.log_table(pos), likelihood.log_table(neg))
    try:
        counts = counted.counts_u32()
        from_sequences = counted.likelihood(table)
        resident = _lib.Batch.from_counts(ctx, counts)
        from_counts = resident.likelihood(table)
        resident.close()
    finally:
        counted.close()
        table.close()
    host = likelihood.score(counts, pos, neg)
    ref.check(host, counts, ref.log_table(pos), ref.log_table(neg), what="counted contigs")
    assert np.array_equal(host, from_sequences) and np.array_equal(host, from_counts)
    indir, data = _write_inputs(tmp_path, seqs, pos, neg)
    sc, cold = _scorer(indir, data)                                  # counts the FASTA file, writes the features cache
    assert np.array_equal(cold, host) and np.array_equal(sc.positive_counts, pos)
    sc, warm = _scorer(indir, data)                                  # starts from the cache's integer rows
    assert sc.features_file and np.array_equal(warm, host)
    _, per_kmer = _scorer(indir, data, likelihood_per_kmer=True, pseudocount=0.25)
    assert np.array_equal(per_kmer, likelihood.score(counts, pos, neg, pseudocount=0.25, per_kmer=True))
    # both strands: queries and references folded alike; a sequence and its reverse complement score the same bits
    _, both = _scorer(indir, data, both_strands=True)
    folded = transform_kmers.fold_strands
    assert np.array_equal(both, likelihood.score(folded(counts.astype(np.int64)), folded(pos), folded(neg)))
    assert not np.array_equal(both, host)
    rc_dir = tmp_path / "rc"
    rc_dir.mkdir()
    indir_rc, _ = _write_inputs(rc_dir, [strands_ref.revcomp(s) for s in seqs], pos, neg)
    _, mirrored = _scorer(indir_rc, data, both_strands=True)
    assert np.array_equal(mirrored, both)
