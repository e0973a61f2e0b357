"""GPU: the density bandwidth sweep (density_sweep.hip) past the shapes of tests/test_gpu_density_sweep.py, held to the
same contract: row b of ``learning.density_sweep(Q, X, hs)`` is bit for bit ``learning.log_density(Q, X, hs[b])``, both are
within 1e-11 x max(1, |want|) of the dense restatement (tests/density_ref.py; leave-one-out rows: tests/density_sweep_ref.py),
and nothing moves under ``_per_pass`` or ``_batch_rows``.

  1. query counts around the blocks of 64 and 128 queries, data rows around the 256-row chunks, D = 32 and D = 33 (the
     guarded loader past one column step of 32), passes of 2 bandwidths (the wide kernel) and of 3 (the narrow one);
  2. ties: rows on a grid of eighths where most queries attain their smallest d^2 twice or more, and rows one ulp apart --
     what the derived running maximum (``mx = -dmin * c``) has to survive;
  3. 10, 11, 16 and 17 bandwidths: later passes of 2 (wide), 3 (narrow), exactly 8, and 8 + 8 + 1;
  4. ``exclude_self`` past one query batch at the guarded width."""
import numpy as np
import pytest

from tests import density_ref, density_sweep_ref

pytestmark = pytest.mark.gpu
F64 = 1e-11
POOL = [0.02, 0.004, 0.05, 0.004, 0.3, 0.0025, 0.01, 0.1, 0.007, 0.03, 0.002, 0.2]


def _bandwidths(B):
    """Unsorted, with a repeated value wherever B >= 4."""
    return [POOL[i % len(POOL)] for i in range(B)]


def ratio(got, want):
    """The largest |got - want| as a share of the bar 1e-11 x max(1, |want|)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.all(np.isfinite(want))
    return float(np.max(np.abs(got - want) / (F64 * np.maximum(1.0, np.abs(want))))) if got.size else 0.0


_singles = {}


def single(tag, Q, X, h):
    """learning.log_density at one bandwidth, once per (input, bandwidth) for the module."""
    from phamers_amd import learning
    if (tag, h) not in _singles:
        _singles[(tag, h)] = learning.log_density(Q, X, h)
    return _singles[(tag, h)]


def assert_sweep(tag, Q, X, hs, variants=((1, 0), (None, 128))):
    """The contract for one input and bandwidth list; returns the worst share of the bar."""
    from phamers_amd import learning
    got = learning.density_sweep(Q, X, hs)
    assert got.shape == (len(hs), len(Q)) and got.dtype == np.float64
    worst = 0.0
    for b, h in enumerate(hs):
        one = single(tag, Q, X, h)
        assert np.array_equal(got[b], one), (tag, len(hs), b, h, np.flatnonzero(got[b] != one)[:8])
        if b == hs.index(h):
            want = density_ref.log_density(Q, X, h)
            worst = max(worst, ratio(got[b], want))
            assert density_ref.close(got[b], want, F64), (tag, len(hs), b, h, ratio(got[b], want))
        else:
            assert np.array_equal(got[b], got[hs.index(h)]), (tag, len(hs), b, h)
    for per, rows in variants:
        assert np.array_equal(learning.density_sweep(Q, X, hs, _per_pass=per, _batch_rows=rows), got), (tag, len(hs), per, rows)
    return worst


# ---- 1. block and chunk edges -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_rows():
    return {D: (density_sweep_ref.smooth_rows(129, D, 12), density_sweep_ref.smooth_rows(513, D, 11)) for D in (32, 33)}


EDGES = [(N, M) for M in (1, 257) for N in (1, 63, 64, 65, 127, 128, 129)] + \
        [(N, M) for N in (65, 129) for M in (255, 256, 513)]      # ((65, 1), (65, 257), (129, 1), (129, 257): in the first list)


@pytest.mark.parametrize("D", [32, 33])
@pytest.mark.parametrize("N,M", EDGES)
def test_block_and_chunk_edges(edge_rows, N, M, D):
    Q, X = edge_rows[D][0][:N], edge_rows[D][1][:M]
    worst = 0.0
    for B in (2, 3):
        worst = max(worst, assert_sweep(("edge", N, M, D), Q, X, _bandwidths(B)))
    print("N = %d, M = %d, D = %d: %.3f of the bar" % (N, M, D, worst))


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------
def _tie_input(case):
    kind, D = case.split("-")
    D = int(D)
    return density_sweep_ref.grid_rows(D, 40 + D) if kind == "grid" else density_sweep_ref.near_tie_rows(D, 50 + D)


@pytest.mark.parametrize("case", ["grid-8", "grid-32", "near-8", "near-32"])
def test_tied_minima_keep_the_single_bandwidth_bits(case):
    """Bit equality with ``log_density`` is the assertion that matters: that path keeps its running maximum, the sweep
    derives it from the running minimum of d^2, and equal or nearly equal d^2 are where the two could part."""
    from phamers_amd import learning
    Q, X = _tie_input(case)
    assert Q.shape[0] == 130 and X.shape[0] == 300
    at_min = density_sweep_ref.rows_at_the_minimum(Q, X)
    if case.startswith("grid"):
        assert 2 * int((at_min >= 2).sum()) >= 130, int((at_min >= 2).sum())
        assert np.array_equal(X[255], X[256]) and np.array_equal(X[16], X[17])
    else:
        d = X[1::2] - X[0::2]
        assert ((d != 0.0).sum(axis=1) == 1).all() and np.abs(d).max() <= 2.0 ** -53
    assert np.array_equal(Q[0], X[16] if case.startswith("grid") else X[0])
    worst = 0.0
    for B in (1, 2, 3, learning.DENSITY_SWEEP_PER_PASS, learning.DENSITY_SWEEP_PER_PASS + 1):
        worst = max(worst, assert_sweep(case, Q, X, _bandwidths(B)))
    print("%s: %d of 130 queries attain their smallest d^2 twice or more; %.3f of the bar" % (case, (at_min >= 2).sum(), worst))


@pytest.mark.parametrize("case", ["grid-8", "grid-32", "near-8", "near-32"])
def test_tied_minima_with_the_own_row_left_out(case):
    from phamers_amd import learning
    _, X = _tie_input(case)
    hs = [0.01, 0.003, 0.05]
    want = density_sweep_ref.log_density_sweep(X, X, hs, exclude_self=True)
    got = learning.density_sweep(X, X, hs, exclude_self=True)
    print("%s, exclude_self: %.3f of the bar" % (case, ratio(got, want)))
    assert density_ref.close(got, want, F64), ratio(got, want)
    for per in (1, 8):
        for rows in (0, 128):
            assert np.array_equal(learning.density_sweep(X, X, hs, exclude_self=True, _per_pass=per, _batch_rows=rows), got), (per, rows)
    if case.startswith("grid"):      # rows 255 and 256 are each other's zero distance: the same density, bit for bit
        assert np.array_equal(got[:, 255], got[:, 256]) and np.array_equal(got[:, 16], got[:, 17])


# ---- 3. pass structure -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["smooth-32", "smooth-33", "grid-8"])
@pytest.mark.parametrize("B", [10, 11, 16, 17])
def test_later_passes_of_every_width(case, B):
    """B = 10: a later pass of 2 bandwidths (the wide kernel after the narrow one); 11: of 3; 16: exactly 8; 17: 8 + 8 + 1."""
    from phamers_amd import learning
    assert learning.DENSITY_SWEEP_PER_PASS == 8
    if case == "grid-8":
        Q, X = _tie_input(case)
    else:
        D = int(case.split("-")[1])
        Q, X = density_sweep_ref.smooth_rows(130, D, 14), density_sweep_ref.smooth_rows(300, D, 13)
    hs = _bandwidths(B)
    assert hs[1] == hs[3] and sorted(hs) != hs
    worst = assert_sweep(case, Q, X, hs)
    print("%s, B = %d: %.3f of the bar" % (case, B, worst))


# ---- 4. exclude_self past one batch at the guarded width ----------------------------------------------------------------
@pytest.mark.parametrize("M", [129, 513])
def test_exclude_self_in_batches_at_the_guarded_width(M):
    """``_batch_rows = 128``: the second and later batches leave out row self0 + q with self0 = 128, 256, ..."""
    from phamers_amd import learning
    X = density_sweep_ref.smooth_rows(M, 33, 15)
    hs = [0.01, 0.003, 0.05]
    want = density_sweep_ref.log_density_sweep(X, X, hs, exclude_self=True)
    got = learning.density_sweep(X, X, hs, exclude_self=True, _batch_rows=128)
    print("M = %d, D = 33, exclude_self in batches of 128: %.3f of the bar" % (M, ratio(got, want)))
    assert density_ref.close(got, want, F64), ratio(got, want)
    assert np.array_equal(learning.density_sweep(X, X, hs, exclude_self=True), got)
    for per in (1, 2):
        assert np.array_equal(learning.density_sweep(X, X, hs, exclude_self=True, _per_pass=per, _batch_rows=128), got), per
    # the row a batch must leave out is its own: with it counted the density at the narrowest bandwidth is far higher
    counted = learning.density_sweep(X, X, hs)
    assert np.all(counted[1] > got[1] + 1.0)
