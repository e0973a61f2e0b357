"""CPU-only: the statement of the S-state chain (tests/compose_ref.py) against its own brute force, the NumPy half of
phamers_amd/compose.py (start rule, M-step) against the statement bit for bit, and ``compose.fit`` driven by the statement
in the place of the device on the "small" sequence."""
import numpy as np
import pytest

from tests import compose_ref as cref

LD = cref.LD


@pytest.fixture
def compose(monkeypatch):
    from phamers_amd import compose as cp
    monkeypatch.setattr(cp, "_estep", cref.StatementEStep)
    return cp


def random_chain(rng, S, low=0.02):
    A = rng.random((S, S)) + low
    pi = rng.random(S) + low
    return A / A.sum(axis=1, keepdims=True), pi / pi.sum()


@pytest.mark.parametrize("S,n", [(2, 1), (2, 7), (3, 2), (3, 5), (3, 6)])
def test_statement_equals_its_brute_force(S, n):
    rng = np.random.default_rng(100 * S + n)
    for trial in range(3):
        E = rng.normal(0.0, 3.0, (n, S)) * (1.0 + 4.0 * trial)
        A, pi = random_chain(rng, S)
        qt, qp = cref.quantise_log(A), cref.quantise_log(pi)
        gamma, xi, g0, le = cref.forward_backward(E, A, pi)
        bg, bxi, ble, best, paths = cref.brute_force(E, A, pi, qt, qp)
        tol = LD(2.0 ** -55)
        assert np.abs(gamma - bg).max() < tol and np.abs(xi - bxi).max() < tol and np.abs(g0 - bg[0]).max() < tol
        assert abs(le - ble) < LD(2.0 ** -50) * (1 + abs(ble))
        states, score = cref.viterbi(cref.quantise(E), qt, qp)
        assert score == best and tuple(int(s) for s in states) in paths
        assert abs(float(gamma.sum()) - n) < 1e-12 and abs(float(xi.sum()) - (n - 1)) < 1e-12


def test_viterbi_tie_rules():
    S = 3
    qt = np.zeros((S, S), dtype=np.int64)
    qp = np.zeros(S, dtype=np.int64)
    states, score = cref.viterbi([[0, 0, 0]] * 5, qt, qp)
    assert states.tolist() == [0] * 5 and score == 0
    # states 1 and 2 equal and better than 0: the end tie goes to 1, every predecessor tie to the smaller state
    states, score = cref.viterbi([[-5, 0, 0]] * 4, qt, qp)
    assert states.tolist() == [1, 1, 1, 1] and score == 0
    # the last window prefers 2; its predecessors tie between 1 and 2 and go to 1
    states, score = cref.viterbi([[-5, 0, 0], [-5, 0, 0], [-5, -1, 0]], qt, qp)
    assert states.tolist() == [1, 1, 2]


def test_quantise_clamps_and_zero_rows():
    E = np.array([[0.0, 0.0], [-1e5, 3.0], [2.5, 2.5 - 2.0 ** -17]])
    assert cref.quantise(E) == [[0, 0], [-(2 ** 31), 0], [0, 0]]      # a tie of rint at half goes to even


def test_start_rule_against_the_statement(compose):
    rng = np.random.default_rng(5)
    profiles = rng.dirichlet(np.ones(16), 3)
    counts = np.vstack([rng.multinomial(60, profiles[(i // 13) % 3]) for i in range(90)]).astype(np.int64)
    counts[20:24] = 0                                   # windows without k-mers inside a block
    counts[40:48] = 0                                   # a whole block (of 4 and of 8) without k-mers
    offsets = np.array([0, 37, 37, 38, 90])
    for block in (4, 8, 20):
        for S in (2, 3, 4):
            logp, idx = compose.start(counts, offsets, S, block, 0.5)
            want, widx = cref.start(counts, offsets, S, block, 0.5)
            assert idx == widx and np.array_equal(logp, want), (block, S)
    P = cref.blocks(counts, offsets, 8)
    assert len(P) == 5 + 0 + 1 + 7 and np.array_equal(P[5], counts[37])          # blocks never cross records
    assert np.array_equal(compose._blocks(counts, offsets, 8), P)
    assert compose.start(counts, offsets, 2, 8)[1][0] == 0
    zero_first = counts.copy()
    zero_first[:8] = 0
    assert compose.start(zero_first, offsets, 2, 8)[1][0] == 1 == cref.start(zero_first, offsets, 2, 8)[1][0]
    with pytest.raises(ValueError):
        compose.start(counts[:8], [0, 8], 3, 4)


def test_m_step_against_the_statement_and_its_rules(compose):
    rng = np.random.default_rng(6)
    S, D = 3, 16
    T, xi, g0 = rng.random((S, D)) * 50, rng.random((S, S)) * 20, rng.random(S)
    A0, pi0 = random_chain(rng, S)
    for prior, mode in ((0.0, 'fixed'), (0.25, 'free'), (rng.random((S, S)), 'free')):
        got = compose.m_step(T, xi, g0, 0.5, prior, mode, A0, pi0)
        want = cref.m_step(T, xi, g0, 0.5, prior, mode, A0, pi0)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    from phamers_amd import mixture
    assert np.array_equal(compose.m_step(T, xi, g0, 0.5)[0], mixture.m_step(T, np.ones(S), 0.5)[0])
    assert compose.m_step(T, xi, g0, 0.5, init=pi0)[2] is pi0
    xi2 = xi.copy()
    xi2[1] = 0.0                                        # a row without expected transitions keeps its values
    xi2[2] = [1.0, 0.0, 1e-20]                          # entries raised to 1e-12, the row normalised again
    A = compose.m_step(T, xi2, g0, 0.5, 0.0, 'fixed', A0, pi0)[1]
    assert np.array_equal(A[1], A0[1]) and A[2].min() >= 1e-12 * (1 - 1e-9) and abs(A[2].sum() - 1.0) <= 2 ** -51
    assert np.array_equal(A[2], (lambda p: p / p.sum())(np.maximum(xi2[2] / xi2[2].sum(), 1e-12)))
    T0 = T.copy()
    T0[0] = 0.0                                         # an empty state gets the uniform profile
    assert np.allclose(np.exp(compose.m_step(T0, xi, g0, 0.5)[0][0]), 1.0 / D, rtol=1e-15)
    with pytest.raises(ValueError):
        compose.m_step(T, xi2, g0, 0.5)                 # nothing to keep
    with pytest.raises(ValueError):
        compose.m_step(T, xi, g0, 0.0)


def test_start_chain(compose):
    A, pi = compose.start_chain(3, 30000, 500)
    assert A[0, 0] == 1 - 500 / 30000.0 and A[0, 1] == A[0, 2] == (1 - A[0, 0]) / 2 and np.array_equal(pi, np.full(3, 1 / 3))
    for S in range(2, 9):
        A, pi = compose.start_chain(S)
        assert np.abs(A.sum(axis=1) - 1).max() <= 2 ** -51 and abs(pi.sum() - 1) <= 2 ** -51
    with pytest.raises(ValueError):
        compose.start_chain(9)
    with pytest.raises(ValueError):
        compose.start_chain(2, 500, 500)


@pytest.fixture(scope="module")
def small():
    return {seed: cref.window_counts(cref.small_sequence(seed)) for seed in (2, 3)}


@pytest.mark.parametrize("seed", [2, 3])
@pytest.mark.parametrize("block", [8, 20])
def test_fit_on_the_small_sequence_with_three_states(compose, small, seed, block):
    C = small[seed]
    comp = compose.fit(C, [0, len(C)], 3, block=block)
    assert comp.converged and comp.n_iter <= 5, comp.n_iter
    assert (np.diff(comp.trace[:, 1]) >= -1e-9 * np.abs(comp.trace[1:, 1])).all()
    dec = comp.decode(C, [0, len(C)])
    assert cref.changes(dec.state) == [12000, 20000, 30000]
    assert dec.state[0] == dec.state[-1] and len(set(dec.state.tolist())) == 3
    assert np.allclose(dec.posterior.sum(axis=1), 1.0, atol=1e-12) and np.isfinite(dec.log_evidence).all()
    assert abs(comp.occupancy.sum() - len(C)) < 1e-9 and np.allclose(comp.expected_counts.sum(axis=0), C.sum(axis=0), rtol=1e-12)
    assert not comp.empty.any() and np.isfinite(comp.bic)
    assert np.array_equal(dec.path_score_q.astype(np.float64) * 2.0 ** -16, dec.path_score)


@pytest.mark.parametrize("seed", [2, 3])
def test_fit_on_the_small_sequence_with_two_states(compose, small, seed):
    C = small[seed]
    comp = compose.fit(C, [0, len(C)], 2)
    assert cref.changes(comp.decode(C, [0, len(C)]).state) == [12000, 30000]


def test_fit_options_and_save_load(compose, small, tmp_path):
    C = small[2]
    off = [0, len(C)]
    kept = compose.fit(C, off, 3, fit_transitions=False, max_iter=2)
    A0, pi0 = compose.start_chain(3)
    assert np.array_equal(kept.trans, A0) and np.array_equal(kept.init, pi0) and kept.n_iter <= 2
    free = compose.fit(C, off, 3, p_start='free', max_iter=1)
    assert not np.array_equal(free.init, pi0) and abs(free.init.sum() - 1) < 1e-15 and free.init.min() >= 1e-12 * (1 - 1e-9)
    by_index = compose.fit(C, off, 3, init=[0, 30, 50], block=1, max_iter=0)
    assert np.array_equal(by_index.log_profiles, np.log((C[[0, 30, 50]] + 0.5) / (C[[0, 30, 50]].sum(axis=1, keepdims=True) + 128.0)))
    by_profile = compose.fit(C, off, 3, init=np.exp(by_index.log_profiles), max_iter=0)
    assert np.allclose(by_profile.log_profiles, by_index.log_profiles, rtol=0, atol=1e-14) and by_profile.n_iter == 0
    path = str(tmp_path / "c.npz")
    kept.save(path)
    back = compose.load(path)
    for name in ("log_profiles", "trans", "init", "occupancy", "expected_counts", "trace"):
        assert np.array_equal(getattr(back, name), getattr(kept, name)), name
    assert (back.temper, back.pseudocount, back.n_iter, back.converged, back.bic) == (
        kept.temper, kept.pseudocount, kept.n_iter, kept.converged, kept.bic)
    for bad in (dict(n_states=1), dict(n_states=9), dict(n_states=3, temper=0.0), dict(n_states=3, pseudocount=0.0),
                dict(n_states=3, p_start='other'), dict(n_states=3, max_iter=-1), dict(n_states=3, init=[0, 1])):
        with pytest.raises(ValueError):
            compose.fit(C, off, **bad)
    owners = np.repeat([0, 1], [50, len(C) - 50])        # owners and offsets are both understood
    assert np.array_equal(compose.fit(C, owners, 2, max_iter=1).log_profiles, compose.fit(C, [0, 50, len(C)], 2, max_iter=1).log_profiles)


def test_label_tells_the_positive_state_on_the_cpu_statement(compose, small, monkeypatch):
    """The expectation the end-to-end GPU test fixes: with the three source rows removed from the references, only the state
    of the second piece (positive row 2200's chain) has a positive per-k-mer likelihood score.  Checked here with the
    float64 statement of the score (log-sum-exp over the reference rows) in the place of the device call."""
    from phamers_amd import likelihood
    from tests import helpers
    g = helpers.load_npz("ref_features.npz")
    pos = np.delete(g["pos_counts"].astype(np.int64), 2200, axis=0)
    neg = np.delete(g["neg_counts"].astype(np.int64), [100, 2000], axis=0)

    def score(rows, p, n, pseudocount=0.5, per_kmer=False):
        rows = np.asarray(rows, dtype=np.float64)
        lse = lambda ref: (lambda S: S.max(axis=1) + np.log(np.exp(S - S.max(axis=1, keepdims=True)).sum(axis=1)) - np.log(len(ref)))(
            rows @ likelihood.log_table(ref, pseudocount).T)
        return (lse(p) - lse(n)) / rows.sum(axis=1)

    monkeypatch.setattr(likelihood, "score", score)
    C = small[2]
    comp = compose.fit(C, [0, len(C)], 3)
    state = comp.decode(C, [0, len(C)]).state
    label = comp.label(pos, neg)
    second = int(state[12000 // 500 + 1])
    assert label[second] > 0 and all(label[s] < 0 for s in range(3) if s != second), label
