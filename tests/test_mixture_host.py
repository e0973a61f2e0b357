"""CPU-only: the statements of tests/mixture_ref.py against each other within the bound, the M-step's rules, the start and stop
rules, ``n_init``, save / load, the command line and the argument errors of phamers_amd/mixture.py with the float64 statement
standing in for the device, and the recovery conditions on the statement alone."""
import os

import numpy as np
import pytest

from tests import mixture_ref as mref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_features.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return z["pos_counts"].astype(np.uint32), z["neg_counts"].astype(np.uint32)


@pytest.fixture()
def mixture(monkeypatch):
    from phamers_amd import mixture as mx
    monkeypatch.setattr(mx, "_estep", mref.StatementEStep)
    return mx


def random_table(rng, K, D, concentration=1.0, dead=()):
    from phamers_amd import mixture as mx
    logp = np.log(rng.dirichlet(np.full(D, concentration), K))
    w = rng.dirichlet(np.ones(K))
    w[list(dead)] = 0.0
    return logp, mx.log_weights(w / w.sum())


# ---- the statements ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,kmers,K,N", [(256, 200, 3, 300), (256, 10 ** 7, 5, 40), (16, 50, 17, 500), (256, 2000, 64, 600),
                                         (256, 300, 2, 2 * mref.BLOCK_ROWS + 1)])
def test_float64_statement_is_inside_the_bound(D, kmers, K, N):
    rng = np.random.RandomState(D + K + N)
    counts = rng.multinomial(kmers, rng.dirichlet(np.ones(D)), N).astype(np.uint32)
    logp, logw = random_table(rng, K, D, dead=(1,) if K > 4 else ())
    got = mref.e_step(counts, logp, logw, np.float64)
    assert mref.check_e_step(got, counts, logp, logw) < 0.5


def test_float64_statement_on_golden_and_awkward_rows(golden):
    from phamers_amd import likelihood
    pos, neg = golden
    longest = neg[np.argsort(neg.sum(axis=1, dtype=np.uint64))[-4:]]
    rows = np.vstack((pos[:50], longest, np.zeros((1, 256), np.uint32), np.eye(1, 256, 7, dtype=np.uint32),
                      np.eye(1, 256, 0, dtype=np.uint32) * 5000))
    logp = likelihood.log_table(np.vstack((pos[100:103], longest[:2], np.eye(1, 256, 0, dtype=np.uint32) * 9000)), 0.5)
    logw = np.log(np.full(6, 1.0 / 6))
    got = mref.e_step(rows, logp, logw, np.float64)
    assert mref.check_e_step(got, rows, logp, logw) < 0.5
    r = got["r"][50:54]                                  # the longest rows: every r is exactly 0 or 1
    assert np.isin(r, (0.0, 1.0)).all() and (r.sum(axis=1) == 1).all()
    assert np.allclose(got["r"][54], np.exp(logw), rtol=1e-14)     # a row without counts: r = pi


def test_tree_sum_is_the_rule_written_out():
    rng = np.random.default_rng(3)
    for R in (1, 2, 255, 256, 257, 1000):
        v = rng.random((R, 3)) * 10.0 ** rng.integers(-3, 4, (R, 1))
        rows = [v[i] for i in range(R)]
        while True:
            blocks = []
            for lo in range(0, len(rows), 256):
                w = rows[lo:lo + 256] + [np.zeros(3)] * (256 - len(rows[lo:lo + 256]))
                s = 128
                while s:
                    w = [w[i] + w[i + s] for i in range(s)]
                    s //= 2
                blocks.append(w[0])
            rows = blocks
            if len(rows) == 1:
                break
        assert np.array_equal(mref.tree_sum(v), rows[0]), R
    assert [mref.tree_levels(b) for b in (1, 256, 257, 65536, 65537)] == [1, 1, 2, 2, 3]
    assert mref.path_additions(1) == mref.BLOCK_ROWS + 8 and mref.path_additions(257 * mref.BLOCK_ROWS) == mref.BLOCK_ROWS + 16


# ---- the M-step -------------------------------------------------------------------------------------------------------------
def test_m_step_rules():
    from phamers_amd import mixture as mx
    rng = np.random.RandomState(0)
    T = rng.gamma(2.0, 50.0, (4, 16))
    T[2] = 0.0
    Nk = np.array([3.0, 5.0, 0.0, 2.0])
    logp, w = mx.m_step(T, Nk, 0.5)
    assert np.allclose(np.exp(logp).sum(axis=1), 1.0, rtol=0, atol=4e-16 * 16)
    assert np.array_equal(logp, np.log((T + 0.5) / (T.sum(axis=1, keepdims=True) + 16 * 0.5)))
    assert np.array_equal(w, Nk / 10.0) and w[2] == 0.0
    assert np.array_equal(logp[2], np.full(16, np.log(0.5 / 8.0)))          # N_k = 0: the pseudocount's uniform profile
    assert mx.log_weights(w)[2] == -np.inf and np.isfinite(mx.log_weights(w)[[0, 1, 3]]).all()
    for bad in (0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            mx.m_step(T, Nk, bad)
    with pytest.raises(ValueError):
        mx.m_step(T, Nk[:3], 0.5)


# ---- start, stop, n_init, files ------------------------------------------------------------------------------------------
def test_start_rule_is_seeded_and_reproducible(mixture):
    from phamers_amd import likelihood
    counts, _ = mref.planted(1, 3, 20, 300, 5.0, D=16)
    e = mref.StatementEStep(counts)
    logp, w = mixture.start(e, 4, 0.5, seed=7)
    index = np.random.RandomState(7).choice(60, 4, replace=False)
    assert np.array_equal(logp, likelihood.log_table(counts[index], 0.5)) and np.array_equal(w, np.full(4, 0.25))
    assert np.array_equal(mixture.start(e, 4, 0.5, seed=7)[0], logp)
    assert np.array_equal(mixture.start(e, 4, 0.5, init=index)[0], logp)
    p = np.random.RandomState(2).dirichlet(np.ones(16), 4)
    assert np.allclose(mixture.start(e, 4, 0.5, init=3.0 * p)[0], np.log(p), rtol=1e-14)
    a = mixture.fit(counts, 3, seed=5)
    b = mixture.fit(counts, 3, seed=5)
    assert np.array_equal(a.log_profiles, b.log_profiles) and np.array_equal(a.trace, b.trace)
    for bad in ([0, 1], [0, 1, 2, 60], [[0.5] * 16] * 3, -np.ones((4, 16))):
        with pytest.raises(ValueError):
            mixture.start(e, 4, 0.5, init=bad)


def test_stop_rule_and_trace(mixture):
    counts, _ = mref.planted(2, 3, 30, 300, 5.0, D=16)
    m = mixture.fit(counts, 3, init=[0, 30, 60], tol=1e-6, max_iter=100)
    F = m.trace[:, 1]
    assert m.converged and m.n_iter == len(F) - 1 and m.n_iter < 100
    gains = np.diff(F)
    assert gains[-1] <= 1e-6 * max(1.0, abs(F[-1])) and (gains[:-1] > 1e-6 * np.maximum(1.0, np.abs(F[1:-1]))).all()
    # the returned parameters are the last row's: its evidence is theirs
    T, Nk, L = m.expect(counts)
    assert L == m.trace[-1, 0] and mixture.evidence(L, m.log_profiles, 0.5) == F[-1]
    assert np.array_equal(m.effective_kmers, T.sum(axis=1)) and not m.dead.any()
    short = mixture.fit(counts, 3, init=[0, 30, 60], tol=0.0, max_iter=2)
    assert not short.converged and short.n_iter == 2 and len(short.trace) == 3
    assert np.array_equal(short.trace[:3], m.trace[:3])
    zero = mixture.fit(counts, 3, init=[0, 30, 60], max_iter=0)
    assert zero.n_iter == 0 and len(zero.trace) == 1 and np.array_equal(zero.weights, np.full(3, 1 / 3.0))


def test_n_init_keeps_the_largest_evidence_lowest_seed_on_ties(mixture):
    counts, _ = mref.planted(3, 4, 15, 150, 20.0, D=16)
    singles = [mixture.fit(counts, 4, seed=10 + i, max_iter=30) for i in range(4)]
    best = mixture.fit(counts, 4, seed=10, n_init=4, max_iter=30)
    finals = [s.trace[-1, 1] for s in singles]
    assert best.trace[-1, 1] == max(finals)
    assert np.array_equal(best.log_profiles, singles[int(np.argmax(finals))].log_profiles)      # argmax: the first = lowest seed
    with pytest.raises(ValueError):
        mixture.fit(counts, 4, init=[0, 1, 2, 3], n_init=2)


def test_save_load_round_trip(mixture, tmp_path):
    counts, _ = mref.planted(4, 2, 20, 200, 5.0, D=16)
    m = mixture.fit(counts, 2, seed=0)
    path = str(tmp_path / "m.npz")
    m.save(path)
    back = mixture.load(path)
    for name in ("log_profiles", "weights", "trace", "effective_kmers", "dead"):
        assert np.array_equal(getattr(m, name), getattr(back, name)), name
    assert (back.pseudocount, back.n_iter, back.converged) == (m.pseudocount, m.n_iter, m.converged)
    assert np.array_equal(back.log_likelihood(counts), m.log_likelihood(counts))


def test_dead_components_are_reported_and_stay_dead(mixture):
    counts, _ = mref.planted(5, 2, 20, 200, 5.0, D=16)
    e = mref.StatementEStep(counts)
    logp, w = mixture.start(e, 3, 0.5, init=[0, 20, 1])
    w = np.array([0.5, 0.5, 0.0])
    got = mixture._em(e, logp, w, 0.5, 20, 1e-9)
    assert got.weights[2] == 0 and np.array_equal(got.log_profiles[2], np.full(16, np.log(1 / 16.0)))
    assert np.isfinite(got.trace[:, :2]).all() and (got.trace[:, 3] == 1).all() and (got.T[2] == 0).all()
    m = mixture.Mixture(got.log_profiles, got.weights, 0.5)
    assert m.dead.tolist() == [False, False, True]
    r = m.responsibilities(counts)
    assert (r[:, 2] == 0).all() and np.allclose(r.sum(axis=1), 1.0)


def test_assign_score_and_from_rows(mixture, golden):
    from phamers_amd import likelihood
    pos, neg = golden
    a, b = mixture.from_rows(pos[:40]), mixture.from_rows(neg[:30])
    q = np.vstack((pos[40:60], neg[30:50]))
    got = mixture.score(q, a, b)
    lp = likelihood.log_table(pos[:40], 0.5), likelihood.log_table(neg[:30], 0.5)
    S = [q.astype(np.longdouble) @ t.T.astype(np.longdouble) for t in lp]
    lse = [s.max(axis=1) + np.log(np.exp(s - s.max(axis=1, keepdims=True)).sum(axis=1)) - np.log(np.longdouble(s.shape[1])) for s in S]
    want = (lse[0] - lse[1]).astype(np.float64)
    assert np.allclose(got, want, rtol=1e-9, atol=1e-6)
    assert np.allclose(mixture.score(q, a, b, per_kmer=True), want / q.sum(axis=1), rtol=1e-9, atol=1e-12)
    # ties go to the lowest index: identical components
    twin = mixture.Mixture(np.vstack((a.log_profiles[:1],) * 3), [0.25, 0.5, 0.25], 0.5)
    comp, resp = twin.assign(q)
    assert (comp == 1).all() and np.allclose(resp, 0.5)
    even = mixture.Mixture(np.vstack((a.log_profiles[:1],) * 3), np.full(3, 1 / 3.0), 0.5)
    assert (even.assign(q)[0] == 0).all()
    with pytest.raises(ValueError):
        mixture.from_rows(pos[:257])


def test_value_errors(mixture, golden):
    pos, _ = golden
    counts = pos[:20]
    with pytest.raises(ValueError, match="not frequencies"):
        mixture.fit(counts / counts.sum(axis=1, keepdims=True), 2)
    for K in (0, 257, -1):
        with pytest.raises(ValueError):
            mixture.fit(counts, K)
    with pytest.raises(ValueError, match="exceeds"):
        mixture.fit(counts, 21)
    for a in (0.0, -0.5, np.nan, np.inf):
        with pytest.raises(ValueError):
            mixture.fit(counts, 2, pseudocount=a)
    for kw in (dict(n_init=0), dict(max_iter=-1), dict(tol=-1.0), dict(tol=np.nan)):
        with pytest.raises(ValueError):
            mixture.fit(counts, 2, **kw)
    m = mixture.fit(counts, 2, seed=0, max_iter=2)
    with pytest.raises(ValueError, match="columns"):
        m.log_likelihood(counts[:, :64])
    with pytest.raises(ValueError, match="not frequencies"):
        mixture.score(counts * 0.5, m, m)


def test_command_line_writes_its_three_files(mixture, golden, tmp_path):
    from phamers_amd import fileIO
    pos, neg = golden
    counts = np.vstack((pos[:30], neg[:30]))
    ids = np.array(["row_%d" % i for i in range(60)])
    features = str(tmp_path / "features.csv")
    fileIO.save_counts(counts, ids, features)
    out = str(tmp_path / "out")
    assert mixture.main(["-in", features, "-K", "3", "--seed", "1", "--max_iter", "25", "-out", out]) == 0
    want = mixture.fit(counts, 3, seed=1, max_iter=25)
    comp = np.loadtxt(os.path.join(out, "mixture_components.csv"), delimiter=",", skiprows=1, ndmin=2)
    assert comp.shape == (3, 4 + 256) and np.array_equal(comp[:, 0], np.arange(3))
    assert np.array_equal(comp[:, 1], want.weights) and np.array_equal(comp[:, 2], want.effective_kmers)
    assert np.array_equal(comp[:, 4:], np.exp(want.log_profiles)) and not comp[:, 3].any()
    with open(os.path.join(out, "mixture_assignments.csv")) as f:
        lines = f.read().splitlines()
    assert lines[0] == "id,component,responsibility,log_likelihood,log_likelihood_per_kmer" and len(lines) == 61
    c, r = want.assign(counts)
    ll = want.log_likelihood(counts)
    for i, line in enumerate(lines[1:]):
        f = line.split(",")
        assert f[0] == ids[i] and int(f[1]) == c[i] and float(f[2]) == r[i] and float(f[3]) == ll[i]
        assert float(f[4]) == ll[i] / counts[i].sum(dtype=np.uint64)
    trace = np.loadtxt(os.path.join(out, "mixture_trace.csv"), delimiter=",", skiprows=1, ndmin=2)
    assert np.array_equal(trace[:, 1:], want.trace) and np.array_equal(trace[:, 0], np.arange(len(want.trace)))
    with pytest.raises(SystemExit):
        mixture.main(["-in", features, "-out", out])


# ---- recovery on the statement alone ---------------------------------------------------------------------------------------
def summed_bound_on_L(counts, log_profiles):
    c = counts.astype(np.float64)
    e = (c.shape[1] + 2) * mref.U * (c @ np.abs(log_profiles).T).max(axis=1)
    K, t = len(log_profiles), mref.path_additions(len(c))
    l_abs = (c @ np.abs(log_profiles).T).max(axis=1) + 50.0                 # |l_i| <= max_k |S| + |log pi| (generous)
    return float((e + (K + 64) * mref.U * (1 + l_abs)).sum() + (t + 2) * mref.U * l_abs.sum())


def test_planted_components_are_recovered(mixture):
    counts, labels = mref.planted(0, 3, 100, 400, 5.0)
    starts = [dict(init=[0, 100, 200])] + [dict(seed=s) for s in range(5)]
    for kw in starts:
        m = mixture.fit(counts, 3, **kw)
        comp, resp = m.assign(counts)
        owner = [np.bincount(comp[labels == k], minlength=3) for k in range(3)]
        assert all(o.max() == 100 for o in owner) and sorted(int(o.argmax()) for o in owner) == [0, 1, 2], kw
        assert m.converged
        slack = 2 * summed_bound_on_L(counts, m.log_profiles)
        assert (np.diff(m.trace[:, 1]) >= -slack).all()
    assert np.array_equal(mixture.fit(counts, 3, init=[0, 100, 200]).assign(counts)[0], labels)


def test_soft_case_is_monotone_and_soft(mixture):
    counts, _ = mref.planted(0, 3, 100, 200, 20.0)
    m = mixture.fit(counts, 3, init=[0, 100, 200], max_iter=50, tol=0.0)
    assert len(m.trace) == 51
    slack = 2 * summed_bound_on_L(counts, m.log_profiles)
    assert (np.diff(m.trace[:, 1]) >= -slack).all()
    assert (m.assign(counts)[1] < 0.999).sum() > 0


# ---- the inputs of tests/test_gpu_mixture.py: the float64 statement is inside the bound on each ---------------------------------
def test_float64_statement_on_the_inputs_of_the_gpu_tests(golden):
    from phamers_amd import likelihood
    from tests import test_gpu_mixture as gpu
    pos, neg = golden
    n = gpu.RB + 1                                           # the GPU tests' ``rows`` fixture
    rows = np.empty((2 * n, 256), dtype=np.uint32)
    rows[0::2], rows[1::2] = pos[:n], neg[:n]
    rows = rows[:2 * gpu.RB + 1]
    cases = [(rows[:300],) + gpu.table_of(rows, K) for K in (1, 2, 15, 16, 17, 64, 255, 256)]
    cases += [(rows[:N],) + gpu.table_of(rows, 17) for N in (1, 127, 128, 129, gpu.RB - 1, gpu.RB, gpu.RB + 1, 2 * gpu.RB + 1)]
    cases += [(rows,) + gpu.table_of(rows, 70), (rows,) + gpu.table_of(rows, 1)]
    cases += [(rows[:300],) + gpu.table_of(rows, 70, dead=d) for d in ((3,), (0, 5, 6, 69))]
    cases.append((rows[:300], np.repeat(gpu.table_of(rows, 1)[0], 5, axis=0), np.log([0.1, 0.4, 0.2, 0.05, 0.25])))
    for D in (4, 16, 64, 1024):
        rng = np.random.RandomState(D)
        counts = np.stack([rng.multinomial(2500, rng.dirichlet(np.full(D, 0.7))) for _ in range(131)]).astype(np.uint32)
        counts[5] = 0
        cases += [(counts,) + gpu.table_of(counts, K, seed=D) for K in (5, 70)]
    odd = gpu.odd_width_rows()
    cases.append((odd,) + gpu.table_of(odd, 7, seed=30))
    longest = neg[np.argsort(neg.sum(axis=1, dtype=np.uint64))[-4:]]
    awkward = np.vstack((np.zeros((1, 256), np.uint32), np.eye(1, 256, 27, dtype=np.uint32),
                         np.eye(1, 256, 0, dtype=np.uint32) * 4997, longest))
    bare = rows[:6].copy()
    bare[:, 0] = 0
    cases.append((awkward, likelihood.log_table(np.vstack((bare, longest[:2])), 0.5),
                  np.log(np.random.RandomState(1).dirichlet(np.full(8, 2.0)))))
    worst = 0.0
    for counts, logp, logw in cases:
        worst = max(worst, mref.check_e_step(mref.e_step(counts, logp, logw, np.float64), counts, logp, logw))
    assert worst < 0.5, worst


# ---- the device's order of N_k and L, written out (mix_expect_body) ------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("N", [1, 3, 4, 5, 1023, 1024, 1025, 2049])
def test_block_sums_is_the_slot_rule_written_out(N, K):
    rng = np.random.default_rng(N + K)
    for v in (rng.random((N, K)) * 10.0 ** rng.integers(-3, 4, (N, 1)), -rng.random(N) * 1e3):
        want = []
        for b in range(0, N, mref.BLOCK_ROWS):
            slots = [np.zeros(v.shape[1:]) for _ in range(4)]
            for i in range(b, min(b + mref.BLOCK_ROWS, N)):
                slots[(i - b) % 4] = slots[(i - b) % 4] + v[i]
            want.append((slots[0] + slots[1]) + (slots[2] + slots[3]))
        got = mref.block_sums(v)
        assert got.shape == (len(want),) + v.shape[1:] and np.array_equal(got, np.array(want))
    assert np.array_equal(mref.block_sums(np.zeros((0, K))), np.zeros((1, K)))


@pytest.mark.parametrize("D,kmers,K,N", [(256, 200, 3, 300), (16, 50, 17, 2 * mref.BLOCK_ROWS + 1)])
def test_device_order_is_inside_the_bound(D, kmers, K, N):
    rng = np.random.RandomState(D + K + N)
    counts = rng.multinomial(kmers, rng.dirichlet(np.ones(D)), N).astype(np.uint32)
    logp, logw = random_table(rng, K, D)
    got = mref.e_step(counts, logp, logw, np.float64)
    Nk, L = mref.device_order(got["r"], got["l"])
    assert mref.check_e_step(dict(Nk=Nk, L=L), counts, logp, logw) < 0.5


@pytest.fixture(scope="module")
def two_levels():
    """The K = 2 case of tests/test_gpu_mixture_levels.py at 257 blocks, with the float64 statement's r and l."""
    N = 256 * mref.BLOCK_ROWS + 1
    counts, logp, logw = mref.two_profile_case(N, 2)
    got = mref.e_step(counts, logp, logw, np.float64)
    return dict(N=N, counts=counts, logp=logp, logw=logw, r=got["r"], l=got["l"], Nk=got["Nk"], L=got["L"])


def test_two_level_inputs_keep_both_components_alive_and_inside_the_bound(two_levels):
    c = two_levels
    Nk, L = mref.device_order(c["r"], c["l"])
    assert (Nk >= c["N"] / 8.0).all(), Nk
    assert mref.tree_levels(-(-c["N"] // mref.BLOCK_ROWS)) == 2 and mref.tree_levels(256) == 1
    assert mref.check_e_step(dict(Nk=Nk, L=L), c["counts"], c["logp"], c["logw"]) < 0.5
    one = mref.two_profile_case(c["N"], 1)                                   # the K = 1 case: the same rows
    assert np.array_equal(one[0], c["counts"]) and one[2][0] == 0.0 and one[1].shape == (1, 4)


def test_device_order_differs_from_every_other_order_on_the_two_level_inputs(two_levels):
    """What shows that the exact equalities of the GPU tests can fail: on their inputs the device's order gives other bits
    than each order a wrong kernel or a wrong statement would give.  (The tree with the two second-level inputs swapped is
    left out: the second level of 257 blocks is the one addition v[0] + v[1], and a + b == b + a in IEEE arithmetic.)"""
    c = two_levels
    r, l = c["r"], c["l"]
    Nk, L = mref.device_order(r, l)
    for k in range(2):
        assert Nk[k] != r[:, k].sum() and Nk[k] != r.sum(axis=0)[k]           # NumPy's own order
        assert Nk[k] != c["Nk"][k]                                            # the float64 statement's block sums
    assert L != l.sum() and L != c["L"]
    first = 256 * mref.BLOCK_ROWS                                             # one level only / the 257th block dropped
    Nk_first, L_first = mref.device_order(r[:first], l[:first])
    assert (Nk != Nk_first).all() and L != L_first
    parts_r, parts_l = mref.block_sums(r), mref.block_sums(l)
    assert len(parts_r) == 257 and np.array_equal(mref.tree_sum(parts_r[:256]), Nk_first)
    assert mref.tree_sum(parts_l[:256]) == L_first
    # blocks anchored one row late move bits too
    assert (Nk != mref.tree_sum(mref.block_sums(np.vstack((np.zeros((1, 2)), r))))).any()


def test_device_order_differs_from_other_joins_on_the_golden_rows(golden):
    """The order statement at the GPU tests' D = 256 shapes (K = 17): the statement's block sums, NumPy's sums and the four
    slots joined in slot order ((0 + 1) + 2) + 3 each give other bits in some component at every N; L, one number, differs
    from at least one of the two plain sums of l."""
    from tests import test_gpu_mixture as gpu
    pos, neg = golden
    n = gpu.RB + 1
    rows = np.empty((2 * n, 256), dtype=np.uint32)
    rows[0::2], rows[1::2] = pos[:n], neg[:n]
    logp, logw = gpu.table_of(rows[:2 * gpu.RB + 1], 17)
    for N in (gpu.RB - 1, gpu.RB, gpu.RB + 1, 2 * gpu.RB + 1):
        got = mref.e_step(rows[:N], logp, logw, np.float64)
        r, l = got["r"], got["l"]
        Nk, L = mref.device_order(r, l)
        blocks = -(-N // gpu.RB)
        steps = np.zeros((blocks * gpu.RB, 17))
        steps[:N] = r
        steps = steps.reshape(blocks, gpu.RB // 4, 4, 17)
        slots = np.zeros((blocks, 4, 17))
        for i in range(gpu.RB // 4):
            slots += steps[:, i]
        in_slot_order = mref.tree_sum(((slots[:, 0] + slots[:, 1]) + slots[:, 2]) + slots[:, 3])
        assert (Nk != in_slot_order).any() and (Nk != got["Nk"]).any() and (Nk != r.sum(axis=0)).any(), N
        assert L != l.sum() or L != got["L"], N
