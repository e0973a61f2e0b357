"""GPU: the likelihood-ranked reference lookup and host prediction (hosts.hip, phamers_amd/hosts.py) against the extended
precision statement (tests/hosts_ref.py) within the bounds derived there, and bit equality -- indices included -- across
batch splits, entry points, strands and runs.  Shapes are the smallest that cross the kernels' boundaries: the query block
is 128, the row chunk 256, a row step 64, a column step 32; lists of 8 entries serve top <= 8, lists of 16 the rest."""
import numpy as np
import pytest

from tests import helpers, hosts_ref as ref

pytestmark = pytest.mark.gpu

MODELS = ("multinomial", "markov")


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
    """One set of random rows for all the D = 256 cases: 300 queries and 513 reference rows, cut as needed, with the
    longdouble products and the per-row sums of |c| |L| of both tables (the bound of a cut is their maximum over its rows)."""
    rng = np.random.default_rng(21)
    q, x = _contigs(rng, 300, 256), _genomes(rng, 513, 256)
    tables = {m: ref.table(x, m) for m in MODELS}
    S = {m: ref.products(q, tables[m]) for m in MODELS}
    absum = {m: q.astype(np.float64) @ np.abs(tables[m]).T for m in MODELS}
    return q, x, S, absum


def _bound(absum, n, m, D=256):
    return (D + 2) * ref.U * absum[:n, :m].max(axis=1)


# ---- 1. query and row shapes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", [1, 5, 8, 9, 15, 16])         # 8 fills the short list, 9 is the first top of the long one
@pytest.mark.parametrize("m", [16, 255, 257, 513])
@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_shapes_against_extended_statement(shapes, n, m, top):
    from phamers_amd import hosts
    q, x, S, absum = shapes
    for model in MODELS:
        r = hosts.rank(q[:n], x[:m], top=top, model=model)
        assert r.z is None and r.p_value is None
        exact = ref.check_ranking(r.indices, r.log_likelihood, S[model][:n, :m], _bound(absum[model], n, m), top,
                                  what="%s N=%d M=%d top=%d" % (model, n, m, top))
        assert exact >= 0.9
        assert np.array_equal(r.per_kmer, r.log_likelihood / 4997.0)


@pytest.mark.parametrize("m", [8, 9])
@helpers.timed
def test_lists_as_long_as_the_table(shapes, m):
    """top = M = 8: every row returned from a full short list; top = M = 9: the long list's first use, with nothing left out."""
    from phamers_amd import hosts
    q, x, S, absum = shapes
    for model in MODELS:
        r = hosts.rank(q[:129], x[:m], top=m, model=model)
        assert (np.sort(r.indices, axis=1) == np.arange(m)).all()
        assert ref.check_ranking(r.indices, r.log_likelihood, S[model][:129, :m], _bound(absum[model], 129, m), m,
                                 what="%s M=top=%d" % (model, m)) >= 0.9


def test_one_row_one_hit(shapes):
    from phamers_amd import hosts
    q, x, S, absum = shapes
    for model in MODELS:
        r = hosts.rank(q[:129], x[:1], top=1, model=model)
        assert (r.indices == 0).all()
        assert ref.check_ranking(r.indices, r.log_likelihood, S[model][:129, :1], _bound(absum[model], 129, 1), 1) == 1.0


# ---- 2. batch splits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", [5, 16])
def test_batch_splits_do_not_change_a_bit(shapes, top):
    from phamers_amd import hosts
    q, x, S, absum = shapes
    for model in MODELS:
        whole = hosts.rank(q, x, top=top, model=model)
        assert ref.check_ranking(whole.indices, whole.log_likelihood, S[model], _bound(absum[model], 300, 513), top) >= 0.9
        for rows in (128, 1):                                      # three batches: 128 + 128 + 44 (1: rounded up to the block)
            split = hosts.rank(q, x, top=top, model=model, _batch_rows=rows)
            assert np.array_equal(whole.indices, split.indices) and np.array_equal(whole.log_likelihood, split.log_likelihood)
        for lo, hi in ((0, 1), (127, 300), (299, 300)):            # nor does N, or where in the call a query stands
            part = hosts.rank(q[lo:hi], x, top=top, model=model)
            assert np.array_equal(whole.indices[lo:hi], part.indices)
            assert np.array_equal(whole.log_likelihood[lo:hi], part.log_likelihood)
        again = hosts.rank(q, x, top=top, model=model)              # run to run
        assert np.array_equal(whole.indices, again.indices) and np.array_equal(whole.log_likelihood, again.log_likelihood)


@pytest.mark.parametrize("top", [5, 16])
@helpers.timed
def test_groups_across_batches_do_not_change_a_bit(shapes, top):
    """Random group ids on both sides and three device batches: every batch must read its own queries' ids.
    (tests/test_hosts_host.py: with the first batch's ids in every batch most later queries get rows of their own group.)"""
    from phamers_amd import hosts
    q, x, S, absum = shapes
    gq, gr = ref.random_groups(4, 300), ref.random_groups(5, 513)
    out = ref.excluded(gq, gr, 300, 513)
    for model in MODELS:
        whole = hosts.rank(q, x, top, model, query_groups=gq, reference_groups=gr, _batch_rows=0)
        assert not out[np.arange(300)[:, None], whole.indices].any()     # never a row of its own group
        assert ref.check_ranking(whole.indices, whole.log_likelihood, S[model], _bound(absum[model], 300, 513), top, out=out,
                                 what="%s groups top=%d" % (model, top)) >= 0.9
        for rows in (128, 1):
            split = hosts.rank(q, x, top, model, query_groups=gq, reference_groups=gr, _batch_rows=rows)
            assert np.array_equal(whole.indices, split.indices) and np.array_equal(whole.log_likelihood, split.log_likelihood)
        part = hosts.rank(q[127:300], x, top, model, query_groups=gq[127:300], reference_groups=gr, _batch_rows=128)
        assert np.array_equal(whole.indices[127:300], part.indices)
        assert np.array_equal(whole.log_likelihood[127:300], part.log_likelihood)


# ---- 3. other widths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 16, 64, 1024])
def test_other_widths_through_a_resident_batch(D):
    """D = 4 and 16 are the widths a batch accepts that are no multiple of the column step: the guarded loader."""
    from phamers_amd import _lib, hosts
    rng = np.random.default_rng(D)
    q, x = _contigs(rng, 131, D, kmers=2500), _genomes(rng, 70, D)
    q[5] = 0
    ctx = _lib.get_context()
    for model in MODELS:
        L = hosts._table(x, model, 0.5)
        table = _lib.HostTable(ctx, L)
        batch = _lib.Batch.from_counts(ctx, q)
        assert batch is not None and batch.D == D
        try:
            idx, s = batch.hosts(table, 5)
            h_idx, h_s = table.rank(q, 5)
        finally:
            batch.close()
            table.close()
        assert ref.check_ranking(idx, s, ref.products(q, L), ref.bound(q, L), 5, what="%s D=%d" % (model, D)) >= 0.9
        assert np.array_equal(idx, h_idx) and np.array_equal(s, h_s)
        r = hosts.rank(q, x, top=5, model=model)
        assert np.array_equal(idx, r.indices) and np.array_equal(s, r.log_likelihood)
        assert r.indices[5].tolist() == [0, 1, 2, 3, 4] and (r.log_likelihood[5] == 0.0).all()


# ---- 4. exact ties -----------------------------------------------------------------------------------------------------------
def test_identical_rows_tie_exactly_across_chunk_borders(shapes):
    from phamers_amd import hosts, likelihood
    q, x, _, _ = shapes
    x = x.copy()
    x[256], x[512] = x[255], x[0]                  # twins in chunks 0 | 1 and 0 | 2
    queries = likelihood.thin(x[[255, 0, 256, 512]], 2000, np.random.RandomState(5))
    for model in MODELS:
        for top in (2, 5, 8, 9, 16):
            r = hosts.rank(queries, x, top=top, model=model)
            for row, (lo, hi) in enumerate(((255, 256), (0, 512), (255, 256), (0, 512))):
                i, s = r.indices[row].tolist(), r.log_likelihood[row]
                assert i[:2] == [lo, hi] and s[0] == s[1], (model, top, row, i, s)       # its own profile first, the twin next
            L = ref.table(x, model)
            ref.check_ranking(r.indices, r.log_likelihood, ref.products(queries, L), ref.bound(queries, L), top)


@helpers.timed
def test_twins_at_the_edge_of_the_short_list(shapes):
    """A query whose ranks 8 and 9 are one profile held by two rows in different chunks: with top = 8 the list ends with the
    lower index of the pair, with top = 9 both come, in index order and with equal S.  Query and pair come from the longdouble
    products: the first query whose first ten gaps all exceed 4 e, its rank-8 row, copied over its least likely row of
    another chunk."""
    from phamers_amd import hosts
    q, x, S, absum = shapes
    for model in MODELS:
        e = _bound(absum[model], 300, 513)
        order = ref.ranking(S[model], 10)[0]
        first = np.take_along_axis(S[model], order, axis=1)
        clear = np.flatnonzero((first[:, :-1] - first[:, 1:]).min(axis=1).astype(np.float64) > 4.0 * e)
        qi = int(clear[0])
        row = int(order[qi, 7])
        elsewhere = np.setdiff1d(np.flatnonzero(np.arange(513) // 256 != row // 256), order[qi])
        victim = int(elsewhere[np.argmin(S[model][qi, elsewhere])])
        y = x.copy()
        y[victim] = x[row]
        lo, hi = min(row, victim), max(row, victim)
        L = ref.table(y, model)
        for top in (8, 9):
            r = hosts.rank(q[qi:qi + 1], y, top=top, model=model)
            i, s = r.indices[0].tolist(), r.log_likelihood[0]
            assert i[:7] == order[qi, :7].tolist() and i[7] == lo, (model, top, i, lo, hi)
            if top == 9:
                assert i[8] == hi and s[7] == s[8], (model, i, s)
            # (its exact-indices statement steps back at the pair's tie; the lines above are that statement here)
            ref.check_ranking(r.indices, r.log_likelihood, ref.products(q[qi:qi + 1], L), ref.bound(q[qi:qi + 1], L), top)


def test_duplicate_genomes_of_the_reference_come_in_index_order(golden):
    from phamers_amd import hosts, likelihood
    neg = golden[1]
    assert np.array_equal(neg[2097], neg[2102])
    queries = np.vstack((likelihood.thin(neg[[2097, 2102]], 4997, np.random.RandomState(1)), neg[2097:2098]))
    for model in MODELS:
        r = hosts.rank(queries, neg, top=5, model=model)
        for row in range(3):
            i = r.indices[row].tolist()
            at = i.index(2097)
            assert at < 4 and i[at + 1] == 2102 and r.log_likelihood[row, at] == r.log_likelihood[row, at + 1], (model, i)
        assert r.indices[2, 0] == 2097                  # the genome itself: no other row is more likely


# ---- 5. edge rows ------------------------------------------------------------------------------------------------------------
def test_edge_rows(golden):
    from phamers_amd import hosts
    pos, neg = golden
    x = neg[:300]
    zero = np.zeros(256, dtype=np.int64)
    one = zero.copy()
    one[27] = 1
    huge = zero.copy()
    huge[200] = 2 ** 32 - 1
    q = np.stack((zero, one, huge))
    for model in MODELS:
        null = hosts.fit_null(pos[:40], x, model=model)
        r = hosts.rank(q, x, top=5, model=model, null=null)
        L = ref.table(x, model)
        S, e = ref.products(q, L), ref.bound(q, L)
        ref.check_ranking(r.indices, r.log_likelihood, S, e, 5, what=model)
        # no counts: rows 0..top-1, S exactly 0, nothing to divide by
        assert r.indices[0].tolist() == [0, 1, 2, 3, 4] and (r.log_likelihood[0] == 0.0).all()
        assert np.isnan(r.per_kmer[0]).all() and np.isnan(r.z[0]).all() and np.isnan(r.p_value[0]).all()
        # one k-mer: S is one table entry, the ranking that column's
        assert np.array_equal(r.log_likelihood[1], L[r.indices[1], 27]) and np.array_equal(r.per_kmer[1], r.log_likelihood[1])
        assert r.indices[1].tolist() == ref.ranking(L[:, 27][None, :], 5)[0][0].tolist()
        # 2^32 - 1 in one bin (an exact float64; within the bound above): the ranking is that column's, n is not rounded
        assert r.indices[2].tolist() == ref.ranking(L[:, 200][None, :], 5)[0][0].tolist()
        assert np.array_equal(r.per_kmer[2], r.log_likelihood[2] / (2.0 ** 32 - 1))
        assert np.isfinite(r.z[1:]).all() and ((r.p_value[1:] >= 0) & (r.p_value[1:] <= 1)).all()


def test_groups(shapes):
    from phamers_amd import hosts
    q, x, S, absum = shapes
    q, x = q[:140], x[:300]
    gq, gr = np.arange(140) % 5 - 1, np.arange(300) % 7 - 1             # some without a group on both sides
    for model in MODELS:
        plain = hosts.rank(q, x, top=16, model=model)
        got = hosts.rank(q, x, top=16, model=model, query_groups=gq, reference_groups=gr)
        out = ref.excluded(gq, gr, 140, 300)
        assert not out[np.arange(140)[:, None], got.indices].any()       # never a row of its own group
        assert ref.check_ranking(got.indices, got.log_likelihood, S[model][:140, :300], _bound(absum[model], 140, 300), 16,
                                 out=out, what=model) >= 0.9
        free = gq < 0                                                    # group -1 excludes nothing
        assert np.array_equal(got.indices[free], plain.indices[free]) and not np.array_equal(got.indices, plain.indices)
        one_side = hosts.rank(q, x, top=16, model=model, query_groups=gq)
        assert np.array_equal(one_side.indices, plain.indices) and np.array_equal(one_side.log_likelihood, plain.log_likelihood)
        # -1 on the reference side is no group either
        loose = hosts.rank(q[:3], x[:6], top=4, model=model, query_groups=[-1, 0, 1], reference_groups=[-1, -1, 0, 0, 1, -1])
        assert sorted(loose.indices[0].tolist()) == sorted(ref.ranking(S[model][:1, :6], 4)[0][0].tolist())
        assert not set(loose.indices[1].tolist()) & {2, 3} and 4 not in loose.indices[2].tolist()
    with pytest.raises(ValueError, match="top = 5 exceeds the 4 reference rows query 1"):
        hosts.rank(q[:2], x[:6], top=5, query_groups=[3, 0], reference_groups=[0, 0, 1, 2, 3, 4])
    hosts.rank(q[:2], x[:6], top=4, query_groups=[3, 0], reference_groups=[0, 0, 1, 2, 3, 4])      # top rows left: served


# ---- 6. the null -------------------------------------------------------------------------------------------------------------
def test_null_on_random_rows(shapes):
    from phamers_amd import hosts
    q, x, _, _ = shapes
    x = x[:257]
    for model in MODELS:
        mu, sigma = hosts.fit_null(q, x, model=model)
        ref.check_null(mu, sigma, q, ref.table(x, model), what="300 x 257 " + model)
        mu2, sigma2 = hosts.fit_null(q, x, model=model, _batch_rows=128)
        assert np.array_equal(mu, mu2) and np.array_equal(sigma, sigma2)
        assert (sigma > 0).all()


def test_null_on_golden_rows_and_the_annotation(golden):
    from phamers_amd import hosts
    pos, neg = golden
    x = neg[:300]
    for model in MODELS:
        mu, sigma = hosts.fit_null(pos, x, model=model)
        ref.check_null(mu, sigma, pos, ref.table(x, model), what="golden phage rows " + model)
        mu2, sigma2 = hosts.fit_null(pos, x, model=model, _batch_rows=128)
        assert np.array_equal(mu, mu2) and np.array_equal(sigma, sigma2)
        q = pos[:50]
        r = hosts.rank(q, x, top=5, model=model, null=(mu, sigma))
        z, p = ref.z_and_p(r.log_likelihood / q.sum(axis=1)[:, None].astype(np.float64), r.indices, mu, sigma)
        assert np.array_equal(r.z, z) and np.array_equal(r.p_value, p)
        both = hosts.predict(q, x, pos, top=5, model=model)
        assert np.array_equal(both.indices, r.indices) and np.array_equal(both.z, r.z) and np.array_equal(both.p_value, p)
    default = hosts.predict(pos[:3], x, pos[:40])                        # predict defaults to the Markov table
    assert np.array_equal(default.log_likelihood, hosts.rank(pos[:3], x, model='markov').log_likelihood)
    assert np.array_equal(hosts.rank(pos[:3], x).indices, hosts.rank(pos[:3], x, model='multinomial').indices)


# ---- 7. entry points ---------------------------------------------------------------------------------------------------------
def _write_inputs(tmp_path, seqs, pos, neg):
    from phamers_amd import fileIO
    data = tmp_path / "data" / "reference_features"
    data.mkdir(parents=True)
    fileIO.save_counts(pos, ["p%d" % i for i in range(len(pos))], str(data / "positive_features.csv"))
    fileIO.save_counts(neg, ["NC_%06d" % i for i in range(len(neg))], str(data / "negative_features.csv"))
    indir = tmp_path / "in"
    indir.mkdir()
    with open(indir / "contigs.fasta", "w") as f:
        for c, s in enumerate(seqs):
            f.write(">SuperContig_%d_length_%d_ID_%d\n" % (c, len(s), c))
            f.write("\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + "\n")
    return indir, tmp_path / "data"


def _scorer(indir, data, top, model, out, **attrs):
    from phamers_amd import phamer
    sc = phamer.phamer_scorer()
    sc.keep_reference_counts = True
    for k, v in attrs.items():
        setattr(sc, k, v)
    sc.input_directory, sc.data_directory, sc.output_directory = str(indir), str(data), str(out)
    sc.find_data_files()
    sc.load_data()
    try:
        r = sc.predict_hosts(top, model)
        sc.make_hosts_file()
        return sc, r
    finally:
        sc._drop_batch()


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_entry_points_agree_bit_for_bit(golden, tmp_path):
    from phamers_amd import _lib, hosts, synth, transform_kmers
    from tests import strands_ref
    pos, neg = golden
    pos, neg = pos[:150], neg[:140]
    seqs = [synth.synth_contig(11, c, 5000 + 37 * c) for c in range(20)]
    ctx = _lib.get_context()
    counted = _lib.Batch.from_sequences(ctx, seqs, 4)
    table = _lib.HostTable(ctx, hosts.markov_log_table(neg))
    try:
        counts = counted.counts_u32()
        from_sequences = counted.hosts(table, 3)
        from_counts = table.rank(counts, 3)
    finally:
        counted.close()
        table.close()
    host = hosts.predict(counts, neg, pos, top=3)
    L = ref.table(neg, 'markov')
    ref.check_ranking(host.indices, host.log_likelihood, ref.products(counts, L), ref.bound(counts, L), 3, what="contigs")
    assert _same(from_sequences, host[:2]) and _same(from_counts, host[:2])
    indir, data = _write_inputs(tmp_path, seqs, pos, neg)
    out = tmp_path / "out"
    out.mkdir()
    sc, cold = _scorer(indir, data, 3, 'markov', out)                 # counts the FASTA file, writes the features cache
    assert _same(cold, host) and np.array_equal(sc.negative_counts, neg)
    assert sc.host_ids.tolist() == [["NC_%06d" % i for i in row] for row in host.indices.tolist()]
    assert np.array_equal(sc.host_indices, host.indices) and np.array_equal(sc.host_z, host.z)
    sc, warm = _scorer(indir, data, 3, 'markov', out)                 # starts from the cache's integer rows
    assert sc.features_file and _same(warm, host)
    _, multi = _scorer(indir, data, 2, 'multinomial', out, pseudocount=0.25)
    assert _same(multi, hosts.predict(counts, neg, pos, top=2, model='multinomial', pseudocount=0.25))
    # both strands: queries and both references folded alike; a sequence and its reverse complement give the same file
    _, both = _scorer(indir, data, 3, 'markov', out, both_strands=True)
    folded = transform_kmers.fold_strands
    assert _same(both, hosts.predict(folded(counts.astype(np.int64)), folded(neg), folded(pos), top=3))
    assert not np.array_equal(both.log_likelihood, host.log_likelihood)
    forward = (out / "phamer_hosts.csv").read_bytes()
    rc_dir = tmp_path / "rc"
    rc_dir.mkdir()
    indir_rc, _ = _write_inputs(rc_dir, [strands_ref.revcomp(s) for s in seqs], pos, neg)
    _, mirrored = _scorer(indir_rc, data, 3, 'markov', out, both_strands=True)
    assert _same(mirrored, both) and (out / "phamer_hosts.csv").read_bytes() == forward
    assert forward.count(b"\n") == 2 + 20 * 3


# ---- 8. the command line -----------------------------------------------------------------------------------------------------
def test_command_line(golden, tmp_path):
    from phamers_amd import fileIO, hosts, kmer, phamer, synth
    pos, neg = golden
    pos, neg = pos[:200], neg[:220]
    seqs = [synth.synth_contig(12, c, 5000 + 17 * c) for c in range(12)]
    indir, data = _write_inputs(tmp_path, seqs, pos, neg)
    argv = ["-in", str(indir), "-data", str(data)]
    out = indir / "phamer_output"
    phamer.main(argv)
    plain = (out / "phamer_scores.csv").read_bytes()
    assert not (out / "phamer_hosts.csv").exists()
    scorer = phamer.main(argv + ["--hosts", "3"])
    assert (out / "phamer_scores.csv").read_bytes() == plain
    contigs = [str(i) for i in scorer.data_ids]
    assert len(contigs) == 12 and contigs == list(fileIO.read_phamer_output(str(out / "phamer_scores.csv")))
    rows = fileIO.read_phamer_hosts(str(out / "phamer_hosts.csv"))
    want = hosts.predict(kmer.count(seqs, 4), neg, pos, top=3)
    assert rows == [(contigs[a], r + 1, "NC_%06d" % want.indices[a, r], float(want.log_likelihood[a, r]),
                     float(want.per_kmer[a, r]), float(want.z[a, r]), float(want.p_value[a, r]))
                    for a in range(12) for r in range(3)]
    text = (out / "phamer_hosts.csv").read_text()
    assert text.startswith("# PhaMers host prediction file\n") and "# hosts:\t3\n" in text and "hosts_model" not in text
    phamer.main(argv + ["--hosts", "2", "--hosts_model", "multinomial"])
    assert (out / "phamer_scores.csv").read_bytes() == plain
    rows = fileIO.read_phamer_hosts(str(out / "phamer_hosts.csv"))
    want = hosts.predict(kmer.count(seqs, 4), neg, pos, top=2, model='multinomial')
    assert [r[2] for r in rows] == ["NC_%06d" % i for i in want.indices.ravel()] and len(rows) == 24
    assert "# hosts_model:\t'multinomial'\n" in (out / "phamer_hosts.csv").read_text()
