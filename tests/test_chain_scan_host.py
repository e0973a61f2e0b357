"""CPU-only: the statement of the tile scan (tests/chain_scan_ref.py) against the sequential
statements of tests/compose_ref.py -- the float64 tile route inside the derived bounds of the longdouble forward-backward,
the integer tile route equal to the sequential max-plus -- and the ``scan`` argument of phamers_amd/compose.py."""
import numpy as np
import pytest

from tests import chain_scan_ref as sref
from tests import compose_ref as cref

T = sref.TILE
LENGTHS = [1, 2, T - 1, T, T + 1, 3 * T + 5, 1000]


def random_chain(rng, S, low=0.02):
    A = rng.random((S, S)) + low
    pi = rng.random(S) + low
    return A / A.sum(axis=1, keepdims=True), pi / pi.sum()


def tiny_chain(S):
    """A with entries of 1e-12 beside its diagonal; rows sum to 1 within an ulp."""
    A = np.full((S, S), 1e-12)
    np.fill_diagonal(A, 1.0 - (S - 1) * 1e-12)
    return A, np.full(S, 1.0 / S)


def emissions(rng, n, S, kind):
    E = rng.normal(0.0, 3.0, (n, S))
    if kind == "underflow":      # exp(d) underflows to 0 for some states, on both sides of every tile edge
        E[rng.random((n, S)) < 0.3] -= 2.0 ** 15 + 500.0
        for edge in range(T, n, T):
            E[edge - 1, 1:] = -40000.0
            E[edge, :-1] = -40000.0
    return E


def compare(E, A, pi, S, what):
    n = len(E)
    gamma, xi, g0, le = cref.forward_backward(E, A, pi)
    got_gamma, got_xi, got_g0, got_le = sref.tile_forward_backward(E, A, pi)
    worst = sref.check_posterior(got_gamma, gamma, n, S, what + " gamma")
    worst = max(worst, sref.check_posterior(got_g0, g0, n, S, what + " gamma0"))
    worst = max(worst, sref.check_sums(got_xi, xi, n, S, n, n, what + " xi"))
    worst = max(worst, sref.check_evidence(got_le, le, E.max(axis=1), S, what + " evidence"))
    return worst


@pytest.mark.parametrize("S", [2, 3, 5, 8])
def test_tile_statement_inside_the_scan_bounds(S):
    rng = np.random.default_rng(40 + S)
    worst = 0.0
    for n in LENGTHS:
        for kind in ("plain", "underflow"):
            E = emissions(rng, n, S, kind)
            worst = max(worst, compare(E, *random_chain(rng, S), S, "S=%d n=%d %s" % (S, n, kind)))
            worst = max(worst, compare(E, *tiny_chain(S), S, "S=%d n=%d %s tiny A" % (S, n, kind)))
    print("S = %d: worst error / bound of the float64 tile statement %.3g" % (S, worst))
    assert worst <= 1.0


def test_bounds_are_the_sequential_ones_plus_the_carry():
    for n, S in [(1, 2), (T, 3), (T + 1, 5), (1000, 8)]:
        K = -(-n // T)
        assert sref.n_tiles(n) == K
        assert sref.scan_posterior_bound(n, S) == cref.posterior_bound(n, S) + 2.0 * K * (2.0 * S + 2.0) * cref.U
        M = np.linspace(-50.0, -1.0, n)
        assert sref.scan_evidence_bound(M, S, -7.0) == cref.evidence_bound(M, S, -7.0) + K * (2.0 * S + 2.0) * cref.U


@pytest.mark.parametrize("S", [2, 3, 5, 8])
def test_tile_max_plus_is_the_sequential_one(S):
    rng = np.random.default_rng(7 + S)
    for n in LENGTHS:
        A, pi = random_chain(rng, S)
        qt, qp = cref.quantise_log(A), cref.quantise_log(pi)
        q = cref.quantise(emissions(rng, n, S, "underflow" if n % 2 else "plain"))
        want, score = cref.viterbi(q, qt, qp)
        got, got_score = sref.tile_viterbi(q, qt, qp)
        assert got_score == score and np.array_equal(got, want), (S, n)
        # coarse integers: ties at almost every step
        q = [[int(v) for v in row] for row in rng.integers(-1, 1, (n, S))]
        zt, zp = np.zeros((S, S), dtype=np.int64), np.zeros(S, dtype=np.int64)
        want, score = cref.viterbi(q, zt, zp)
        got, got_score = sref.tile_viterbi(q, zt, zp)
        assert got_score == score and np.array_equal(got, want), (S, n, "ties")


def test_tile_max_plus_all_ties():
    S, n = 3, 3 * T + 5
    zt, zp = np.zeros((S, S), dtype=np.int64), np.zeros(S, dtype=np.int64)
    states, score = sref.tile_viterbi([[0] * S] * n, zt, zp)
    assert states.tolist() == [0] * n and score == 0
    # a tie placed at a tile's last and first step: states 1 and 2 equal and better than 0 there
    q = [[0] * S for _ in range(n)]
    q[T - 1], q[T] = [-5, 0, 0], [-5, 0, 0]
    q[2 * T] = [-5, -1, 0]
    want, score = cref.viterbi(q, zt, zp)
    got, got_score = sref.tile_viterbi(q, zt, zp)
    assert got_score == score and np.array_equal(got, want)


def test_scan_argument():
    from phamers_amd import compose
    assert compose._scan(None) == compose._scan(False) == compose._scan(0) == 0
    assert compose._scan(True) == compose.SCAN_FROM and compose.SCAN_FROM >= 1
    assert compose.SCAN_FROM & (compose.SCAN_FROM - 1) == 0          # a power of two
    assert compose._scan(1) == 1 and compose._scan(np.int64(77)) == 77
    for bad in (-1, 1.5, "yes", [4], 2 ** 64):
        with pytest.raises(ValueError):
            compose._scan(bad)
    C = np.ones((4, 16), dtype=np.uint32)
    with pytest.raises(ValueError):        # refused before anything is made resident
        compose.fit(C, [0, 4], 2, scan=-3)
    comp = compose.Composition(np.log(np.full((2, 16), 1.0 / 16)), [[0.9, 0.1], [0.1, 0.9]], [0.5, 0.5])
    with pytest.raises(ValueError):
        comp.decode(C, [0, 4], scan="all")
    with pytest.raises(ValueError):
        compose.segment_sequences(["ACGT" * 300], 2, scan=2.5)
    args = compose._parser().parse_args(["-in", "x.fa", "-out", "o", "-S", "2"])
    assert args.scan is None
    assert compose._parser().parse_args(["-in", "x.fa", "-out", "o", "-S", "2", "--scan"]).scan is True
    assert compose._parser().parse_args(["-in", "x.fa", "-out", "o", "-S", "2", "--scan", "128"]).scan == 128
    for bad in ("0", "-4"):
        with pytest.raises(SystemExit):
            compose.main(["-in", "x.fa", "-out", "o", "-S", "2", "--scan", bad])
