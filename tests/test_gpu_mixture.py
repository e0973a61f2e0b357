"""GPU: the mixture E-step (mixture.hip) and the fit around it (phamers_amd/mixture.py) against the extended-precision
statement of tests/mixture_ref.py within the bound stated there, and bit equality of T, N_k, L and the row outputs across
batch splits, entry points and runs.  Shapes are the smallest that cross the kernels' boundaries: the row block of the first
product is 128, its component step 64, the column step 32; the second product takes 64 components x 64 columns per wave, four
column tiles per workgroup, and reduces in blocks of 1024 rows."""
import os

import numpy as np
import pytest

from tests import helpers, likelihood_ref as lref, mixture_ref as mref

pytestmark = pytest.mark.gpu
RB = mref.BLOCK_ROWS


@pytest.fixture(scope="module")
def golden():
    g = helpers.load_npz("ref_features.npz")
    return g["pos_counts"].astype(np.uint32), g["neg_counts"].astype(np.uint32)


@pytest.fixture(scope="module")
def rows(golden):
    """2 * RB + 1 golden rows, phage and bacterial alternating: every D = 256 case cuts its rows from these."""
    pos, neg = golden
    n = RB + 1
    out = np.empty((2 * n, 256), dtype=np.uint32)
    out[0::2], out[1::2] = pos[:n], neg[:n]
    return out[:2 * RB + 1]


def table_of(rows, K, seed=0, dead=()):
    """K smoothed golden rows as profiles (picked across the rows) and Dirichlet weights; ``dead``: weights of exactly 0."""
    from phamers_amd import likelihood, mixture
    rng = np.random.RandomState(seed + K)
    logp = likelihood.log_table(rows[rng.choice(len(rows), K, replace=False)], 0.5)
    w = rng.dirichlet(np.full(K, 2.0))
    w[list(dead)] = 0.0
    return logp, mixture.log_weights(w / w.sum())


def e_step(counts, logp, logw, batch_rows=0, resident=False):
    """dict(T, Nk, L, l, argmax, max_resp) of one device E-step from host counts or through a resident batch."""
    from phamers_amd import _lib
    ctx = _lib.get_context()
    table = _lib.MixtureTable(ctx, logp, logw)
    batch = _lib.Batch.from_counts(ctx, counts) if resident else None
    try:
        out = batch.mixture_expect(table, batch_rows, rows=True) if resident else table.expect(counts, batch_rows, rows=True)
    finally:
        if batch is not None:
            batch.close()
        table.close()
    return dict(zip(("T", "Nk", "L", "l", "argmax", "max_resp"), out))


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("T", "Nk", "L", "l", "argmax", "max_resp"))


def check_responsibilities(counts, logp, logw, **kw):
    """r from the device within r (rho + 2u) of the extended statement's; argmax and max_resp are r's."""
    from phamers_amd import _lib
    table = _lib.MixtureTable(_lib.get_context(), logp, logw)
    try:
        r, ll = table.responsibilities(counts)
    finally:
        table.close()
    exact = mref.e_step(counts, logp, logw)
    b = mref.bounds(counts, logp, exact)
    want = exact["r"].astype(np.float64)
    assert (np.abs(r - want) <= want * (b["rho"][:, None] + 2 * mref.U) + mref.TINY).all()
    got = e_step(counts, logp, logw, **kw)
    assert np.array_equal(ll, got["l"])
    assert np.array_equal(got["argmax"], np.argmax(r, axis=1)) and np.array_equal(got["max_resp"], r.max(axis=1))
    return r


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 15, 16, 17, 64, 255, 256])
def test_components_against_extended_statement(rows, K):
    counts = rows[:300]
    logp, logw = table_of(rows, K)
    got = e_step(counts, logp, logw)
    assert got["T"].shape == (K, 256) and got["Nk"].shape == (K,) and got["l"].shape == (300,)
    print("K=%d worst error / bound: %.4f" % (K, mref.check_e_step(got, counts, logp, logw)))
    check_responsibilities(counts, logp, logw)


@pytest.mark.parametrize("N", [1, 127, 128, 129, RB - 1, RB, RB + 1, 2 * RB + 1])
def test_rows_against_extended_statement(rows, N):
    counts = rows[:N]
    logp, logw = table_of(rows, 17)
    got = e_step(counts, logp, logw)
    print("N=%d worst error / bound: %.4f" % (N, mref.check_e_step(got, counts, logp, logw)))
    assert same(got, e_step(counts, logp, logw, resident=True))


@pytest.mark.parametrize("D", [4, 16, 64, 1024])
def test_other_widths_through_a_resident_batch(D):
    """D = 4 and 16 take the guarded loader of the first product and leave most lanes of the second without a column."""
    rng = np.random.RandomState(D)
    counts = np.stack([rng.multinomial(2500, rng.dirichlet(np.full(D, 0.7))) for _ in range(131)]).astype(np.uint32)
    counts[5] = 0
    for K in (5, 70):
        logp, logw = table_of(counts, K, seed=D)
        got = e_step(counts, logp, logw, resident=True)
        print("D=%d K=%d worst error / bound: %.4f" % (D, K, mref.check_e_step(got, counts, logp, logw)))
        assert same(got, e_step(counts, logp, logw))


def odd_width_rows(D=30, n=1100):
    rng = np.random.RandomState(D)
    return np.stack([rng.multinomial(800, rng.dirichlet(np.full(D, 0.7))) for _ in range(n)]).astype(np.uint32)


def test_a_width_no_batch_holds_goes_up_from_the_host():
    """D = 30 is no power of 4 and no multiple of 4: host counts on every call, the scalar loaders of both products."""
    from phamers_amd import _lib, mixture
    counts = odd_width_rows()
    assert _lib.Batch.from_counts(_lib.get_context(), counts) is None
    logp, logw = table_of(counts, 7, seed=30)
    got = e_step(counts, logp, logw)
    print("D=30 worst error / bound: %.4f" % mref.check_e_step(got, counts, logp, logw))
    assert same(got, e_step(counts, logp, logw, batch_rows=RB))
    check_responsibilities(counts[:200], logp, logw)
    a = mixture.fit(counts, 3, seed=1, max_iter=5)
    b = mixture.fit(counts, 3, seed=1, max_iter=5, _batch_rows=RB)
    assert np.array_equal(a.trace, b.trace) and np.array_equal(a.log_profiles, b.log_profiles) and len(a.trace) >= 2


def test_one_component_is_exact(rows):
    from phamers_amd import _lib
    logp, logw = table_of(rows, 1)
    assert logw[0] == 0.0
    got = e_step(rows, logp, logw)
    batch = _lib.Batch.from_counts(_lib.get_context(), rows)
    try:
        sums = batch.column_sums()
    finally:
        batch.close()
    assert np.array_equal(got["T"][0], sums.astype(np.float64)) and got["Nk"][0] == float(len(rows))
    assert (got["max_resp"] == 1.0).all() and (got["argmax"] == 0).all()
    assert (check_responsibilities(rows[:200], logp, logw) == 1.0).all()


# ---- 2. the same bits --------------------------------------------------------------------------------------------------------
def test_splits_entry_points_and_runs_do_not_change_a_bit(rows):
    from phamers_amd import _lib
    logp, logw = table_of(rows, 70)
    whole = e_step(rows, logp, logw)
    mref.check_e_step(whole, rows, logp, logw)
    for batch_rows in (RB, 2 * RB, 1):                       # three batches, two, and 1 rounded up to the block
        assert same(whole, e_step(rows, logp, logw, batch_rows=batch_rows))
        assert same(whole, e_step(rows, logp, logw, batch_rows=batch_rows, resident=True))
    assert same(whole, e_step(rows, logp, logw))             # run to run
    # a batch counted from sequences
    rng = np.random.RandomState(9)
    seqs = ["".join(rng.choice(list("ACGT"), int(rng.randint(300, 900)), p=rng.dirichlet(np.full(4, 3.0)))) for _ in range(RB + 40)]
    ctx = _lib.get_context()
    batch = _lib.Batch.from_sequences(ctx, seqs, 4)
    table = _lib.MixtureTable(ctx, logp, logw)
    try:
        counts = batch.counts_u32()
        from_sequences = dict(zip(("T", "Nk", "L", "l", "argmax", "max_resp"), batch.mixture_expect(table, rows=True)))
        r_batch = batch.mixture_responsibilities(table)[0]
    finally:
        batch.close()
        table.close()
    assert same(from_sequences, e_step(counts, logp, logw, batch_rows=RB))
    assert np.array_equal(r_batch, check_responsibilities(counts, logp, logw))


# ---- 3. awkward rows and tables ------------------------------------------------------------------------------------------
def test_awkward_rows(golden, rows):
    from phamers_amd import likelihood
    pos, neg = golden
    longest = neg[np.argsort(neg.sum(axis=1, dtype=np.uint64))[-4:]]
    zero = np.zeros((1, 256), np.uint32)
    counts = np.vstack((zero, np.eye(1, 256, 27, dtype=np.uint32), np.eye(1, 256, 0, dtype=np.uint32) * 4997, longest))
    bare = rows[:6].copy()
    bare[:, 0] = 0                                            # the homopolymer's column comes from the pseudocount alone
    logp = likelihood.log_table(np.vstack((bare, longest[:2])), 0.5)
    logw = np.log(np.random.RandomState(1).dirichlet(np.full(8, 2.0)))
    got = e_step(counts, logp, logw)
    mref.check_e_step(got, counts, logp, logw)
    r = check_responsibilities(counts, logp, logw)
    assert np.allclose(r[0], np.exp(logw), rtol=1e-14, atol=0)            # no counts: r = pi
    assert np.isin(r[3:], (0.0, 1.0)).all() and (r[3:].sum(axis=1) == 1).all()   # exp(-10^7) is 0, not NaN
    assert got["l"][3:].max() < -1e6 and np.isfinite(got["T"]).all()
    alone = e_step(zero, logp, logw)                                        # adds nothing to T and pi to N_k
    assert not alone["T"].any() and np.allclose(alone["Nk"], np.exp(logw), rtol=1e-14)


@pytest.mark.parametrize("dead", [(3,), (0, 5, 6, 69)])
def test_components_of_weight_zero_contribute_nothing(rows, dead):
    counts = rows[:300]
    logp, logw = table_of(rows, 70, dead=dead)
    assert np.isneginf(logw[list(dead)]).all()
    got = e_step(counts, logp, logw)
    mref.check_e_step(got, counts, logp, logw)
    r = check_responsibilities(counts, logp, logw)
    assert np.isfinite(r).all() and np.isfinite(got["l"]).all()
    assert not got["T"][list(dead)].any() and not got["Nk"][list(dead)].any() and not r[:, list(dead)].any()
    live = [k for k in range(70) if k not in dead]                         # and the rest is the mixture without them
    less = e_step(counts, logp[live], logw[live])
    assert np.allclose(less["l"], got["l"], rtol=1e-12) and np.allclose(less["Nk"], got["Nk"][live], rtol=1e-9, atol=1e-300)


def test_identical_components_share_by_weight(rows):
    counts = rows[:300]
    logp = np.repeat(table_of(rows, 1)[0], 5, axis=0)
    w = np.array([0.1, 0.4, 0.2, 0.05, 0.25])
    got = e_step(counts, logp, np.log(w))
    mref.check_e_step(got, counts, logp, np.log(w))
    r = check_responsibilities(counts, logp, np.log(w))
    b = mref.bounds(counts, logp, dict(l=np.zeros(300), r=np.repeat(w[None, :], 300, axis=0)))   # the exact r is pi itself
    assert (np.abs(r - w[None, :]) <= w[None, :] * (b["rho"][:, None] + 2 * mref.U)).all() and (got["argmax"] == 1).all()
    assert (np.abs(got["T"] - w[:, None] * counts.sum(axis=0, dtype=np.uint64)[None, :]) <= b["T"]).all()
    assert (np.abs(got["Nk"] - 300 * w) <= b["Nk"]).all()


# ---- 4. the fit ------------------------------------------------------------------------------------------------------------
def test_planted_fit_on_the_device_follows_the_statement(monkeypatch):
    from phamers_amd import mixture
    counts, labels = mref.planted(0, 3, 100, 400, 5.0)
    fitted = mixture.fit(counts, 3, init=[0, 100, 200])
    monkeypatch.setattr(mixture, "_estep", mref.StatementEStep)
    stated = mixture.fit(counts, 3, init=[0, 100, 200])
    monkeypatch.undo()
    assert fitted.converged and np.array_equal(fitted.assign(counts)[0], labels)
    shared = min(len(fitted.trace), len(stated.trace))
    assert shared >= 2
    for i in range(shared):                                   # F within the summed bound on L of the statement's
        c = counts.astype(np.float64)
        S_abs = c @ np.abs(stated.log_profiles).T
        e = 258 * mref.U * S_abs.max(axis=1)
        l_abs = S_abs.max(axis=1) + 50.0
        bound = (e + (3 + 64) * mref.U * (1 + l_abs)).sum() + (mref.path_additions(300) + 2) * mref.U * l_abs.sum()
        assert abs(fitted.trace[i, 1] - stated.trace[i, 1]) <= bound, i
    assert not fitted.dead.any() and np.allclose(fitted.effective_kmers.sum(), 300 * 400, rtol=1e-12)


def test_fit_is_bit_for_bit_across_batch_rows_and_runs():
    from phamers_amd import _lib, mixture
    counts, _ = mref.planted(1, 3, 700, 200, 20.0)
    kw = dict(init=[0, 700, 1400], max_iter=6, tol=0.0)
    a = mixture.fit(counts, 3, **kw)
    b = mixture.fit(counts, 3, _batch_rows=RB, **kw)
    batch = _lib.Batch.from_counts(_lib.get_context(), counts)
    try:
        c = mixture.fit(batch, 3, **kw)
        d = mixture.fit(batch, 3, seed=3, n_init=2, max_iter=4)
        e = mixture.fit(counts, 3, seed=3, n_init=2, max_iter=4, _batch_rows=2 * RB)
    finally:
        batch.close()
    for other in (b, c, mixture.fit(counts, 3, **kw)):
        assert np.array_equal(a.trace, other.trace) and np.array_equal(a.log_profiles, other.log_profiles)
        assert np.array_equal(a.weights, other.weights) and np.array_equal(a.effective_kmers, other.effective_kmers)
    assert len(a.trace) == 7 and (np.diff(a.trace[:, 1]) > 0).all()
    assert np.array_equal(d.trace, e.trace) and np.array_equal(d.log_profiles, e.log_profiles)


def test_score_against_the_likelihood_method_and_ties(golden):
    from phamers_amd import likelihood, mixture
    pos, neg = golden
    q = np.vstack((pos[200:400], neg[200:400]))
    a, b = mixture.from_rows(pos[:200]), mixture.from_rows(neg[:200])
    got = mixture.score(q, a, b)
    want = likelihood.score(q, pos[:200], neg[:200])
    lp, ln = a.log_profiles, b.log_profiles
    bound = 0.0
    for logp, mix in ((lp, a), (ln, b)):
        exact = mref.e_step(q, logp, np.log(mix.weights))
        bound = bound + mref.bounds(q, logp, exact)["l"]
    ext = lref.statement(q, lp, ln, dtype=np.longdouble)
    bound = bound + lref.tolerance(q, lp, ln, ext[0], ext[1])
    assert (np.abs(got - want) <= bound).all()
    assert np.array_equal(mixture.score(q, a, b, per_kmer=True), got / q.sum(axis=1, dtype=np.uint64).astype(np.float64))
    twin = mixture.Mixture(np.vstack((lp[:1],) * 4), np.full(4, 0.25), 0.5)
    comp, resp = twin.assign(q)
    assert (comp == 0).all() and np.allclose(resp, 0.25, rtol=1e-12)
    tilted = mixture.Mixture(np.vstack((lp[:1],) * 4), [0.2, 0.3, 0.3, 0.2], 0.5)
    assert (tilted.assign(q)[0] == 1).all()


# ---- 5. the command line and the refusals --------------------------------------------------------------------------------
def test_command_line_on_a_fasta_file_and_on_a_features_file(tmp_path):
    from phamers_amd import fileIO, kmer, mixture
    rng = np.random.RandomState(4)
    comps = ([0.35, 0.15, 0.15, 0.35], [0.15, 0.35, 0.35, 0.15])
    fasta = str(tmp_path / "contigs.fasta")
    with open(fasta, "w") as f:
        for i in range(40):
            seq = "".join(rng.choice(list("ACGT"), 1500 + 10 * i, p=comps[i % 2]))
            f.write(">SuperContig_%d_length_%d_ID_%d\n%s\n" % (i, len(seq), i, seq))
    out = str(tmp_path / "from_fasta")
    assert mixture.main(["-in", fasta, "-K", "2", "-k", "3", "--seed", "0", "-out", out]) == 0
    ids, counts = kmer.count_file(fasta, 3)
    features = str(tmp_path / "features.csv")
    fileIO.save_counts(counts, ids, features)
    out2 = str(tmp_path / "from_features")
    assert mixture.main(["-in", features, "-K", "2", "--seed", "0", "-out", out2]) == 0
    for name in ("mixture_components.csv", "mixture_assignments.csv", "mixture_trace.csv"):
        with open(os.path.join(out, name)) as f1, open(os.path.join(out2, name)) as f2:
            assert f1.read() == f2.read(), name
    want = mixture.fit(counts, 2, seed=0)
    comp = np.loadtxt(os.path.join(out, "mixture_components.csv"), delimiter=",", skiprows=1, ndmin=2)
    assert comp.shape == (2, 4 + 64) and np.array_equal(comp[:, 1], want.weights)
    with open(os.path.join(out, "mixture_assignments.csv")) as f:
        lines = f.read().splitlines()[1:]
    assert [line.split(",")[0] for line in lines] == [str(i) for i in ids]
    assigned = np.array([int(line.split(",")[1]) for line in lines])
    assert np.array_equal(assigned, want.assign(counts)[0])
    assert len(set(assigned[0::2])) == 1 and len(set(assigned[1::2])) == 1 and assigned[0] != assigned[1]


def test_refusals(rows):
    from phamers_amd import _lib, mixture
    ctx = _lib.get_context()
    logp, logw = table_of(rows, 3)
    for bad_p, bad_w in ((np.where(np.arange(256) == 3, -np.inf, logp), logw), (np.where(np.arange(256) == 3, np.nan, logp), logw),
                         (logp, [0.0, np.nan, 0.0]), (logp, [0.0, np.inf, 0.0]), (logp, [-np.inf] * 3), (logp, logw[:2])):
        with pytest.raises(ValueError):
            _lib.MixtureTable(ctx, bad_p, bad_w)
    with pytest.raises(ValueError):
        _lib.MixtureTable(ctx, np.zeros((257, 16)) - 3.0, np.zeros(257))
    table = _lib.MixtureTable(ctx, logp, logw)
    try:
        with pytest.raises(ValueError):
            table.expect(rows[:10, :64])
        with pytest.raises(ValueError):
            table.update(logp[:2], logw[:2])
        with pytest.raises(ValueError):
            table.update(logp, [0.0, np.nan, 0.0])
        T, Nk, L = table.expect(np.zeros((0, 256), np.uint32))
        assert not T.any() and not Nk.any() and L == 0.0
        table.update(logp, logw)
        mref.check_e_step(dict(zip(("T", "Nk", "L"), table.expect(rows[:50]))), rows[:50], logp, logw)
    finally:
        table.close()
    with pytest.raises(ValueError):
        table.expect(rows[:10])                               # closed
    with pytest.raises(ValueError, match="not frequencies"):
        mixture.fit(rows[:20] / 7.0, 2)
    for K in (0, 257):
        with pytest.raises(ValueError):
            mixture.fit(rows[:300], K)
    with pytest.raises(ValueError):
        mixture.fit(rows[:5], 6)
