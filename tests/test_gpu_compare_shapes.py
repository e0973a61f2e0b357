"""The paired comparison on the device (phk_compare_*, phamers_amd/csrc/evaluate.hip) past the shapes tests/test_gpu_compare.py
reaches: Gram sums that need all 64 bits and the refusal one step further, every cell-tile count the header allows, row
chunks at exact multiples and with one class nearly empty, the bootstrap with more than one cell group, a first resample other
than 0 and the default launch split.  Every quantity is an integer (or one rounding of an exact rational), so every assertion
is equality with the statement tests/compare_ref.py -- its sort-based placements and chunked Grams where the P x N matrix
would not fit (tests/test_compare_host.py checks those against the brute-force forms)."""
import numpy as np
import pytest

from tests import compare_ref as ref

pytestmark = pytest.mark.gpu

SMALL = (37, 45)
TILE, GRAM_ROWS, GRAM_STEP, BOOT_CELLS, BOOT_PER_LAUNCH = 32, 256, 64, 8, 1024   # CMP_* of evaluate.hip


def _assert_delong_equals_statement(d, st, covariance=True):
    assert d.placements_positive.dtype == np.uint32 and np.array_equal(d.placements_positive, st.t_pos)
    assert d.placements_negative.dtype == np.uint32 and np.array_equal(d.placements_negative, st.t_neg)
    assert d.area2 == st.area2 and all(isinstance(a, int) for a in d.area2)
    assert d.gram_positive.dtype == np.uint64 and np.array_equal(d.gram_positive.astype(object), st.G10)
    assert d.gram_negative.dtype == np.uint64 and np.array_equal(d.gram_negative.astype(object), st.G01)
    assert np.array_equal(d.covariance, d.covariance.T) and np.isfinite(d.covariance).all()
    if covariance:
        assert d.covariance.shape == (st.C, st.C) and np.array_equal(d.covariance, st.covariance())   # bit for bit


def _delong_against_statement(scores, P):
    from phamers_amd import compare
    st = ref.Statement(scores, P, by_sort=True)
    d = compare.delong(scores, P)
    _assert_delong_equals_statement(d, st)
    return d, st


# ---- 1. Gram sums past 32 bits -------------------------------------------------------------------------------------------------
def test_gram_sums_past_32_bits():
    P, N = 2000, 2100
    scores = ref.noisy_cells(np.random.RandomState(41), P, N, 3)
    assert scores.shape == (3, P + N)
    _, st = _delong_against_statement(scores, P)
    assert max(int(v) for v in st.G10.ravel()) >= 2 ** 32 and max(int(v) for v in st.G01.ravel()) >= 2 ** 32
    brute = ref.Statement(scores, P)                      # (this shape still fits the P x N form: the two statements agree)
    assert brute.area2 == st.area2 and np.array_equal(brute.G10, st.G10) and np.array_equal(brute.G01, st.G01)


def test_one_workgroups_own_sums_pass_32_bits():
    """The sums above pass 2^32 only once the row chunks are added up.  With a fully separated cell every positive's
    placement is 2 N, so the 256 rows of one workgroup alone sum to 256 (2 N)^2 >= 2^32: the registers must be wide too."""
    P, N = 2000, 2100
    rng = np.random.RandomState(42)
    assert GRAM_ROWS * (2 * N) ** 2 >= 2 ** 32 and GRAM_ROWS * (2 * P) ** 2 < 2 ** 32
    scores = np.vstack((np.r_[rng.uniform(1, 2, P), rng.uniform(-2, -1, N)], ref.noisy_cells(rng, P, N, 1)))
    _, st = _delong_against_statement(scores, P)
    assert int(st.G10[0][0]) == 4 * N * N * P and int(st.G01[0][0]) == 4 * P * P * N


# ---- 2. ... past 2^63, at the exactness limit ----------------------------------------------------------------------------------
def test_gram_sums_past_2_to_63():
    """4 N^2 P = 1.058e19 and 4 P^2 N = 1.021e19: both in [2^63, 2^64), where a signed or a float accumulator fails.  Cell 0
    is fully separated (every t_pos = 2 N, every t_neg = 2 P: the Gram diagonals in closed form), cell 1 noisy with ties."""
    P, N = 1350000, 1400000
    assert 2 ** 63 <= 4 * N * N * P < 2 ** 64 and 2 ** 63 <= 4 * P * P * N < 2 ** 64
    rng = np.random.RandomState(43)
    scores = np.empty((2, P + N))
    scores[0] = np.r_[rng.uniform(1, 2, P), rng.uniform(-2, -1, N)]
    scores[1] = np.round(np.r_[np.ones(P), np.zeros(N)] + rng.normal(0, 1, P + N), 3)
    d, st = _delong_against_statement(scores, P)
    assert int(st.G10[0][0]) == 4 * N * N * P >= 2 ** 63 and int(st.G01[0][0]) == 4 * P * P * N >= 2 ** 63
    assert int(d.gram_positive[0, 0]) == 4 * N * N * P and int(d.gram_negative[0, 0]) == 4 * P * P * N
    assert st.area2[0] == 2 * P * N and 0 < st.area2[1] < 2 * P * N
    assert len(np.unique(scores[1])) < (P + N) // 100                          # ties, and many per value
    assert int(st.G10[1][1]) >= 2 ** 62 and int(st.G10[0][1]) >= 2 ** 62       # the noisy cell's sums are of that size too
    assert d.covariance[0, 0] == 0.0 and d.covariance[1, 1] > 0.0              # a separated cell has no variance


# ---- 3. one step over the limit --------------------------------------------------------------------------------------------------
def test_one_row_per_class_past_the_limit_is_refused_and_the_context_lives_on():
    from phamers_amd import _lib, compare
    N = int(round(2.0 ** (62.0 / 3.0)))
    while 4 * N ** 3 >= 2 ** 64:
        N -= 1
    N += 1                                                 # the smallest P = N with 4 N^2 P >= 2^64
    assert 4 * (N - 1) ** 3 < 2 ** 64 <= 4 * N ** 3 and 2 * N < 2 ** 31
    ctx = _lib.get_context()
    scores = np.zeros((1, 2 * N))                          # the check comes before any launch, but the rows are really there
    with pytest.raises(ValueError, match="exact below"):
        _lib.Compare(ctx, scores, N)
    with pytest.raises(ValueError, match="exact below"):
        compare.delong(scores, N)
    P, M = SMALL
    small = ref.noisy_cells(np.random.RandomState(44), P, M, 3)
    h = _lib.Compare(ctx, small, P)                        # the same context still serves a valid call
    try:
        st = ref.Statement(small, P)
        t_pos, t_neg = h.placements()
        area2, g10, g01 = h.grams()
        assert np.array_equal(t_pos, st.t_pos) and np.array_equal(t_neg, st.t_neg) and area2.tolist() == st.area2
        assert np.array_equal(g10.astype(object), st.G10) and np.array_equal(g01.astype(object), st.G01)
        assert np.array_equal(h.bootstrap(3, 2), ref.bootstrap_brute(small, P, 3, 2))
    finally:
        h.close()


# ---- 4. cell tiles up to the header's limit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,shape", [(64, SMALL), (96, SMALL), (97, SMALL), (255, SMALL), (256, SMALL), (256, (130, 70))],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_cell_tiles_to_the_limit(C, shape):
    """2, 3, 4 (one cell in the last) and 8 tiles of 32 cells: 3, 6, 10 and 36 tile pairs through the triangular decode."""
    from phamers_amd import _lib
    assert _lib.COMPARE_MAX_CELLS == 256
    P, N = shape
    scores = ref.noisy_cells(np.random.RandomState(200 + C + P), P, N, C)
    assert scores.shape == (C, P + N)
    d, st = _delong_against_statement(scores, P)
    brute = ref.grams(*ref.placements(scores, P))
    assert brute[0] == st.area2 and np.array_equal(brute[1], st.G10) and np.array_equal(brute[2], st.G01)
    assert len({tuple(r) for r in st.t_pos.tolist()}) >= C - 1   # distinct cells (but the duplicate): a wrong tile would show
    assert np.array_equal(d.gram_positive, d.gram_positive.T) and np.array_equal(d.gram_negative, d.gram_negative.T)


# ---- 5. row chunks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(256, 512), (64, 257), (2, 1000), (1000, 2), (257, 255)], ids=lambda s: "%dx%d" % s)
def test_row_chunks_at_multiples_and_lopsided_classes(shape):
    """Exact multiples of the 256-row chunk and of the 64-row stage, one row past them, and a class of two rows beside one
    of four chunks (three of the small class's four workgroups return at once)."""
    P, N = shape
    scores = ref.noisy_cells(np.random.RandomState(300 + P), P, N, 33)
    _delong_against_statement(scores, P)


# ---- 6. the bootstrap with more than one cell group -----------------------------------------------------------------------------
def _distinct_cells(P, N, C, seed):
    """C cells no two of which are equal: noisy_cells without its closing duplicate."""
    return ref.noisy_cells(np.random.RandomState(seed), P, N, C + 1)[:C]


@pytest.mark.parametrize("C,shape", [(C, s) for s in (SMALL, (301, 212)) for C in (8, 9, 16, 17, 20)] + [(256, SMALL)],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_bootstrap_cell_groups(C, shape):
    """One, two (one cell in the second), two full, three and 32 groups of 8 cells."""
    from phamers_amd import compare
    P, N = shape
    scores = _distinct_cells(P, N, C, 400 + C)
    assert scores.shape == (C, P + N)
    want = ref.bootstrap_runs(scores, P, 6, 3)
    if shape == SMALL:
        assert np.array_equal(want, ref.bootstrap_brute(scores, P, 6, 3))
    assert len({tuple(col) for col in want.T.tolist()}) == C       # a cell written at another cell's place would show
    got = compare.bootstrap(scores, P, resamples=3, seed=6)
    assert got.area2.dtype == np.uint64 and got.area2.shape == (3, C) and np.array_equal(got.area2, want)


# ---- 7. the first resample and the launch split ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def boot_handle():
    from phamers_amd import _lib
    P, N = SMALL
    scores = _distinct_cells(P, N, 9, 500)
    h = _lib.Compare(_lib.get_context(), scores, P)
    yield h, scores, P
    h.close()


@pytest.mark.parametrize("first", [1, 7, 2 ** 32 + 3])
def test_bootstrap_from_a_first_resample(boot_handle, first):
    h, scores, P = boot_handle
    want = ref.bootstrap_runs(scores, P, 11, 6, first=first)
    assert not np.array_equal(want, ref.bootstrap_runs(scores, P, 11, 6))
    assert np.array_equal(h.bootstrap(11, 6, first=first), want)
    if first < 100:
        assert np.array_equal(want, ref.bootstrap_runs(scores, P, 11, first + 6)[first:])   # rows f .. f + count - 1


def test_bootstrap_first_resample_across_launches(boot_handle):
    h, scores, P = boot_handle
    want = ref.bootstrap_runs(scores, P, 11, 45)[5:]
    assert np.array_equal(h.bootstrap(11, 40, first=5, per_launch=16), want)      # launches of 16, 16 and 8 from 5, 21, 37
    assert np.array_equal(h.bootstrap(11, 40, first=5), want)


def test_bootstrap_past_the_default_launch_split(boot_handle):
    h, scores, P = boot_handle
    count = BOOT_PER_LAUNCH + 6
    want = ref.bootstrap_runs(scores, P, 12, count)
    got = h.bootstrap(12, count)
    assert got.shape == (count, 9) and np.array_equal(got, want)
    assert len({tuple(r) for r in want[BOOT_PER_LAUNCH - 3:].tolist()}) == 9       # the rows around the split differ
    assert np.array_equal(h.bootstrap(12, 5, per_launch=1), got[:5])
