"""GPU parity of the row kernels -- normalise (int, float, device pointer, resident batch), widen, the count checker, row and
column gathers, column sums, the host column permutation -- bit for bit against NumPy and exact integer arithmetic, at every
k = 1 .. 7, at odd widths, past one pass of the grid-stride loops (50 001 rows and more: three passes on anything below
1 000 CUs) and past one 256 MiB slice of a download.

References: oracle.normalize_counts (the reference's scripts/kmer.py:209-221, i.e. NumPy itself) and NumPy indexing and
integer sums on the host matrix.  Every comparison is for equality of bits; NaN positions are compared separately.

What the normalise tests pin of phk_div_row (phk_common.h): the division as a whole -- the first quotient x * (1 / T) alone
misrounds on about a quarter of these pairs, a reciprocal approximation on more.  They do not pin its second Newton step:
for integer operands below 2^53 the quotient after one step is already the rounded one (see the comment there).

Left to tests/test_gpu_fullsize.py: the launch split of phk_batch_from_counts and of phk_rowsum_kernel's caller above
2^24 rows (no matrix of that many rows is built here)."""
import ctypes
import os

import numpy as np
import pytest

from tests import helpers, rows_ref

pytestmark = pytest.mark.gpu

U32 = 2 ** 32 - 1
ALL_WIDTHS = tuple(sorted(set(rows_ref.WIDTHS + rows_ref.POW4)))


@pytest.fixture(scope="module")
def kmer():
    from phamers_amd import kmer
    return kmer


@pytest.fixture(scope="module")
def lib():
    from phamers_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    return lib.get_context()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle
    return oracle


def assert_same_bits(got, want, what=""):
    assert got.dtype == np.float64 and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions", np.argwhere(gn != wn)[:5])
    g, w = got[~gn].view(np.uint64), want[~wn].view(np.uint64)
    if not np.array_equal(g, w):
        bad = np.argwhere((got.view(np.uint64) != want.view(np.uint64)) & ~gn)
        raise AssertionError("%s: %d of %d values differ in bits, first at %s: got %r, want %r" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def distinct_pairs(M):
    """A lower bound on the distinct (entry, row sum) pairs of an integer matrix: the distinct entries of every row whose
    sum no other row has."""
    s = M.sum(axis=1)
    _, inv, cnt = np.unique(s, return_inverse=True, return_counts=True)
    solo = cnt[inv.reshape(-1)] == 1
    srt = np.sort(M[solo], axis=1)
    return int((np.diff(srt, axis=1) != 0).sum() + solo.sum())


def big_matrix(n, D, seed, top_bits=25):
    """n rows of random counts whose scale differs from row to row (2^4 .. 2^top_bits), zero rows at 1, n // 2 and n - 1."""
    rng = np.random.default_rng([seed, n, D])
    hi = 2 ** rng.integers(4, top_bits + 1, (n, 1))
    M = (rng.random((n, D)) * hi).astype(np.int64)
    M[[1, n // 2, n - 1]] = 0
    return M


# ---- the four normalise entry points ----------------------------------------------------------------------------------
def norm_device(ctx, M):
    from phamers_amd import device
    n, D = M.shape
    d_in = device.DeviceArray.from_host(ctx, M.astype(np.uint32))
    d_out = device.DeviceArray(ctx, (n, D), np.float64)
    device.normalize(ctx, d_in, n, D, d_out)
    out = d_out.to_host()
    d_in.free()
    d_out.free()
    return out


def norm_batch(lib, ctx, M):
    b = lib.Batch.from_counts(ctx, M)
    assert b is not None
    try:
        return b.normalized()
    finally:
        b.close()


@pytest.mark.parametrize("D", ALL_WIDTHS)
def test_normalize_int64_every_width(kmer, oracle, D):
    """kmer.normalize_counts on int64: row sums 2^m - 1, 2^m, 2^m + 1 up to 2^52, the boundary 2^53 - 1, primes, zero rows,
    entries of 2^32 - 1, negative entries, and 1, 3, 4, 5 rows."""
    rng = np.random.default_rng(D)
    M = rows_ref.division_rows(D, 52, 2 ** 53, max_sum=2 ** 53 - 1, every=4 if D > 8192 else 1)
    M = np.vstack([M, rows_ref.row_with_sum(rng, D, 2 ** 53 - 1, 2 ** 53)[None, :]])
    assert int(M[-1].sum()) == 2 ** 53 - 1
    assert_same_bits(kmer.normalize_counts(M), oracle.normalize_counts(M), "D=%d" % D)
    neg = rng.integers(-5000, 5000, (7, D))
    neg[3] = 0
    neg[5] = -np.abs(neg[5])
    assert_same_bits(kmer.normalize_counts(neg), oracle.normalize_counts(neg), "negative entries, D=%d" % D)
    for n in (1, 3, 4, 5):
        sub = M[rng.choice(len(M), n, replace=False)]
        assert_same_bits(kmer.normalize_counts(sub), oracle.normalize_counts(sub), "%d rows, D=%d" % (n, D))
    got1 = kmer.normalize_counts(M[0])
    assert got1.shape == (D,)
    assert_same_bits(got1, oracle.normalize_counts(M[0]), "1-D")


@pytest.mark.parametrize("D", (2, 3, 4, 64, 65, 256, 8193))
def test_normalize_int64_zero_sum_row_with_entries(kmer, oracle, D):
    """[1, -1, 0, ..] sums to zero: NumPy gives [inf, -inf, nan, ..].  (The Newton-step division alone gives NaN throughout:
    with y = 1 / 0 = inf its residual fma(-inf, 0, x) is NaN.)"""
    M = np.zeros((3, D), dtype=np.int64)
    M[0, :2] = (3, 4)
    M[1, 0], M[1, D - 1] = 1, -1
    M[2, :2] = (5, 6)
    want = oracle.normalize_counts(M)
    assert np.isposinf(want[1, 0]) and np.isneginf(want[1, D - 1]) and (D == 2 or np.isnan(want[1, 1]))
    assert_same_bits(kmer.normalize_counts(M), want, "D=%d" % D)


@pytest.mark.parametrize("D", ALL_WIDTHS)
def test_normalize_float_every_width(kmer, oracle, D):
    """kmer.normalize_counts on float64: NumPy's own summation order and division (magnitudes over six decades; -0.0; zero
    sums; inf), the integer division rows as floats, and 1, 3, 4, 5 rows."""
    F = rows_ref.float_rows(D, 12 if D <= 8192 else 40)
    assert_same_bits(kmer.normalize_counts(F), oracle.normalize_counts(F), "D=%d" % D)
    S = rows_ref.float_special_rows(D)
    assert_same_bits(kmer.normalize_counts(S), oracle.normalize_counts(S), "special rows, D=%d" % D)
    M = rows_ref.division_rows(D, 52, 2 ** 53, max_sum=2 ** 53 - 1, every=4 if D > 8192 else 1).astype(np.float64)
    assert_same_bits(kmer.normalize_counts(M), oracle.normalize_counts(M), "integer-valued rows, D=%d" % D)
    for n in (1, 3, 4, 5):
        assert_same_bits(kmer.normalize_counts(F[:n]), oracle.normalize_counts(F[:n]), "%d rows, D=%d" % (n, D))
    assert_same_bits(kmer.normalize_counts(F[0]), oracle.normalize_counts(F[0]), "1-D")


@pytest.mark.parametrize("k", range(1, 8))
def test_normalize_device_pointer_every_k(ctx, oracle, k):
    """device.normalize (phk_normalize_dev) on uint32 counts: row sums up to 2^32 + 1 (2^46 - 16 384 at D = 16 384: the kernel
    sums in 64 bits), rows of nothing but 2^32 - 1."""
    D = 4 ** k
    M = rows_ref.division_rows(D, 46 if k == 7 else 33, U32)
    assert M.max() == U32 and (k == 1 or int(M.sum(axis=1).max()) > 2 ** 32)
    assert_same_bits(norm_device(ctx, M), oracle.normalize_counts(M), "k=%d" % k)
    rng = np.random.default_rng(k)
    for n in (1, 3, 4, 5):
        sub = M[rng.choice(len(M), n, replace=False)]
        assert_same_bits(norm_device(ctx, sub), oracle.normalize_counts(sub), "%d rows, k=%d" % (n, k))


@pytest.mark.parametrize("k", range(1, 8))
def test_normalize_resident_batch_every_k(lib, ctx, oracle, k):
    """Batch.normalized (phk_batch_normalized): row sums up to 2^32 - 1, the largest a batch holds."""
    D = 4 ** k
    M = rows_ref.division_rows(D, 32, U32, max_sum=U32)
    assert int(M.sum(axis=1).max()) == U32
    assert_same_bits(norm_batch(lib, ctx, M), oracle.normalize_counts(M), "k=%d" % k)
    rng = np.random.default_rng(k)
    for n in (1, 3, 4, 5):
        sub = M[rng.choice(len(M), n, replace=False)]
        assert_same_bits(norm_batch(lib, ctx, sub), oracle.normalize_counts(sub), "%d rows, k=%d" % (n, k))


@pytest.mark.parametrize("D", (16, 64))
def test_normalize_50001_rows_all_entry_points(kmer, lib, ctx, oracle, D):
    """Three passes and more of the grid-stride loop with an odd remainder, and over 2 * 10^6 distinct (entry, row sum) pairs
    through each integer entry point."""
    n = 50001
    M = big_matrix(n, D, seed=1)
    want = oracle.normalize_counts(M)
    assert np.isnan(want[[1, n // 2, n - 1]]).all() and not np.isnan(want[[0, 2, n // 2 - 1, n // 2 + 1, n - 2]]).any()
    assert_same_bits(kmer.normalize_counts(M), want, "int64")
    assert_same_bits(norm_device(ctx, M), want, "device pointer")
    assert_same_bits(norm_batch(lib, ctx, M), want, "resident batch")
    assert_same_bits(kmer.normalize_counts(M.astype(np.float64)), want, "float, integer-valued")
    F = rows_ref.float_rows(D, n)
    F[[1, n - 1]] = 0.0
    assert_same_bits(kmer.normalize_counts(F), oracle.normalize_counts(F), "float")
    if D == 64:
        # the int64 path alone takes sums above 2^32: its own matrix, scales up to 2^45 per entry
        W = big_matrix(n, D, seed=2, top_bits=45)
        assert_same_bits(kmer.normalize_counts(W), oracle.normalize_counts(W), "int64, wide entries")
        pairs = distinct_pairs(M)
        print("distinct (entry, row sum) pairs at 50 001 x 64: >= %d per entry point" % pairs)
        assert pairs >= 2 * 10 ** 6 and distinct_pairs(W) >= 2 * 10 ** 6


@pytest.mark.parametrize("k,n", ((7, 2048 + 37), (6, 8192 + 5)))
def test_download_takes_a_second_slice(lib, ctx, oracle, k, n):
    """Batch.counts / Batch.normalized come down in slices of 256 MiB: 2 048 rows at k = 7, 8 192 at k = 6."""
    D = 4 ** k
    assert n * D * 8 > 256 << 20
    rng = np.random.default_rng(k)
    M = rng.integers(0, 3000, (n, D))
    M[[0, n - 1], 5] = U32 - 3000 * D          # large entries in the first and in the last row
    M[n - 2] = 0
    b = lib.Batch.from_counts(ctx, M)
    assert b is not None and (b.n, b.D) == (n, D)
    try:
        assert np.array_equal(b.counts(), M)
        assert np.array_equal(b.counts_u32(), M.astype(np.uint32))
        assert np.array_equal(batch_rowsums(lib, ctx, b).astype(np.int64), M.sum(axis=1))
        assert_same_bits(b.normalized(), oracle.normalize_counts(M), "k=%d" % k)
        if k == 7:
            assert np.array_equal(b.column_sums(), M.sum(axis=0))
    finally:
        b.close()


# ---- the checker ------------------------------------------------------------------------------------------------------
def poke(ctx, darr, r, j, value):
    """One uint32 word of a device matrix."""
    v = np.array([value], dtype=np.uint32)
    D = darr.shape[1]
    from phamers_amd import _lib
    _lib.check(ctx.lib.phk_memcpy_h2d(ctx.handle, ctypes.c_void_p(darr.ptr + (int(r) * D + int(j)) * 4), _lib.ptr(v), 4))


@pytest.mark.parametrize("n,D", ((100003, 16), (20001, 256), (4100, 16384)))
def test_check_counts_reports_planted_defects(ctx, n, D):
    """device.check_counts is what the full-size tests trust: a clean pair gives (0, 0), one word + 1 gives (1, 1), two words
    of a row swapped give (0, 2), without an expected row sum no row is reported -- in the first and the last row, the last
    word of the matrix, and rows of every pass of the grid-stride loop (4 x 16 blocks per CU: 16 384 rows a pass on 256
    CUs); 1 000 defects are reported as exactly 1 000.  (4 100 x 16 384 is one pass on such a part: that shape is there for
    the wide row, 256 words a lane; the later passes are the other two shapes'.)"""
    from phamers_amd import device
    rng = np.random.default_rng(n)
    A = rng.integers(1, 1000, (n, D), dtype=np.uint32)
    E = 1000 * D + 5
    A[:, 0] = E - A[:, 1:].sum(axis=1, dtype=np.int64)
    assert (A.sum(axis=1, dtype=np.int64) == E).all()
    d_a, d_b = device.DeviceArray.from_host(ctx, A), device.DeviceArray.from_host(ctx, A)
    try:
        assert device.check_counts(ctx, d_a, d_b, n, D, E) == (0, 0)
        assert device.check_counts(ctx, d_a, d_b, n, D, None) == (0, 0)
        assert device.check_counts(ctx, d_a, None, n, D, E) == (0, 0)
        assert device.check_counts(ctx, d_a, None, n, D, E + 1) == (n, 0)
        rows = sorted(set([0, 1, 3, 4, 5, n - 1, n - 2, n - 4, n - 5, n // 2] +
                          [r for r in (4095, 4096, 8191, 8192, 16383, 16384, 16385, 32768, 49152, 65536, 98304) if r < n] +
                          [int(r) for r in rng.integers(0, n, 6)]))
        for r in rows:
            j = D - 1 if r == n - 1 else int(rng.integers(0, D))
            poke(ctx, d_a, r, j, int(A[r, j]) + 1)
            assert device.check_counts(ctx, d_a, d_b, n, D, E) == (1, 1), (r, j)
            assert device.check_counts(ctx, d_a, d_b, n, D, None) == (0, 1), (r, j)
            assert device.check_counts(ctx, d_a, None, n, D, E) == (1, 0), (r, j)
            poke(ctx, d_a, r, j, int(A[r, j]))
            j2 = (j + 1 + int(rng.integers(0, D - 1))) % D
            if A[r, j] != A[r, j2]:
                poke(ctx, d_a, r, j, int(A[r, j2]))
                poke(ctx, d_a, r, j2, int(A[r, j]))
                assert device.check_counts(ctx, d_a, d_b, n, D, E) == (0, 2), (r, j, j2)
                poke(ctx, d_a, r, j, int(A[r, j]))
                poke(ctx, d_a, r, j2, int(A[r, j2]))
        assert device.check_counts(ctx, d_a, d_b, n, D, E) == (0, 0)
        flat = rng.choice(n * D, 1000, replace=False)
        for f in flat:
            poke(ctx, d_a, f // D, f % D, int(A[f // D, f % D]) + 1)
        assert device.check_counts(ctx, d_a, d_b, n, D, E) == (len(set(int(f) // D for f in flat)), 1000)
        assert device.check_counts(ctx, d_a, d_b, n, D, None) == (0, 1000)
        assert device.check_counts(ctx, d_b, d_a, n, D, E) == (0, 1000)     # the defects are in `other`: its row sums are not checked
    finally:
        d_a.free()
        d_b.free()


# ---- resident-batch operations ----------------------------------------------------------------------------------------
def batch_rowsums(lib, ctx, b):
    """The device row sums of a batch (phk_batch_device_ptrs + phk_memcpy_d2h)."""
    d_counts, d_sums = ctypes.c_void_p(), ctypes.c_void_p()
    lib.check(ctx.lib.phk_batch_device_ptrs(b.handle, ctypes.byref(d_counts), ctypes.byref(d_sums)))
    out = np.zeros(b.n, dtype=np.uint32)
    if b.n:
        lib.check(ctx.lib.phk_memcpy_d2h(ctx.handle, lib.ptr(out), d_sums, b.n * 4))
    return out


def assert_batch_is(lib, ctx, b, M, what):
    assert (b.n, b.D) == M.shape, what
    got = b.counts()
    assert got.dtype == np.int64 and np.array_equal(got, M), what
    got32 = b.counts_u32()
    assert got32.dtype == np.uint32 and np.array_equal(got32, M.astype(np.uint32)), what
    assert np.array_equal(batch_rowsums(lib, ctx, b).astype(np.int64), M.sum(axis=1)), what + ": row sums"


def counts_matrix(n, D, seed):
    """Random counts for Batch.from_counts: column 0 stays below 2^17 (a constant gather table on it cannot overflow a row
    sum), some rows hold one entry that brings the row's sum to 2^32 - 1 or close, one row is 2^32 - 1 alone."""
    rng = np.random.default_rng([seed, n, D])
    M = rng.integers(0, 2 ** 17, (n, D))
    M[rng.integers(0, n, n // 5)] //= 4099
    for r in range(2, n, 7):
        j = 1 + int(rng.integers(0, D - 1))
        M[r, j] = 0
        M[r, j] = U32 - int(M[r].sum()) - (r % 3)
    M[n // 2] = 0
    M[n // 2, D - 1] = U32
    M[n - 3] = 0
    assert M.max() == U32 and int(M.sum(axis=1).max()) == U32 and M.min() >= 0
    return M


def batches(lib, ctx, oracle, k):
    """(name, batch, host matrix) both ways: counted from synthetic contigs, and uploaded from a random count matrix."""
    from phamers_amd import synth
    rng = np.random.default_rng(k)
    lens = [0, 1, k - 1, k, k + 1, 31, 32, 33, 64, 1000, 2999] + [int(x) for x in rng.integers(0, 3000, 26)]
    seqs = [synth.synth_contig(21, i, L, invalid_ppm=(0 if i % 4 else 20000)) for i, L in enumerate(lens)]
    yield "from_sequences", lib.Batch.from_sequences(ctx, seqs, k), oracle.count(seqs, k)
    M = counts_matrix(45, 4 ** k, seed=k)
    b = lib.Batch.from_counts(ctx, M)
    assert b is not None
    yield "from_counts", b, M


@pytest.mark.parametrize("k", range(1, 8))
def test_batch_operations_every_k(lib, ctx, oracle, k):
    D = 4 ** k
    rng = np.random.default_rng(100 + k)
    for name, b, M in batches(lib, ctx, oracle, k):
        what = "%s k=%d" % (name, k)
        n = len(M)
        try:
            assert_batch_is(lib, ctx, b, M, what)
            assert_same_bits(b.normalized(), oracle.normalize_counts(M), what)
            sums = b.column_sums()
            assert sums.dtype == np.int64 and np.array_equal(sums, M.sum(axis=0)), what
            # row selections: repeats, descending order, the empty one, a selection of a selection
            idx = np.sort(rng.integers(0, n, 2 * n + 3))[::-1]
            s1 = b.select(idx)
            assert_batch_is(lib, ctx, s1, M[idx], what + " select")
            idx2 = rng.integers(0, len(idx), 17)
            s2 = s1.select(idx2)
            assert_batch_is(lib, ctx, s2, M[idx][idx2], what + " select of select")
            s0 = b.select(np.zeros(0, dtype=np.uint64))
            assert_batch_is(lib, ctx, s0, M[:0], what + " empty select")
            assert s0.normalized().shape == (0, D) and np.array_equal(s0.column_sums(), np.zeros(D, dtype=np.int64))
            for s in (s0, s1, s2):
                s.close()
            # column gathers: a permutation, the identity, a constant table, an arbitrary table of small columns
            for tname, table in (("permutation", rng.permutation(D)), ("identity", np.arange(D)),
                                 ("constant", np.zeros(D, dtype=np.int64))):
                g = b.gather_columns(table)
                assert_batch_is(lib, ctx, g, M[:, table], what + " gather " + tname)
                assert_same_bits(g.normalized(), oracle.normalize_counts(M[:, table]), what + " gather " + tname)
                g.close()
        finally:
            b.close()


def test_select_40001_rows_at_k2(lib, ctx):
    M = counts_matrix(301, 16, seed=5)
    b = lib.Batch.from_counts(ctx, M)
    rng = np.random.default_rng(6)
    idx = np.sort(rng.integers(0, 301, 40001))[::-1].copy()
    idx[:3], idx[-3:] = (300, 300, 0), (0, 300, 150)
    s = b.select(idx)
    assert_batch_is(lib, ctx, s, M[idx], "40 001 rows")
    s2 = s.select(np.arange(40000, -1, -1))
    assert_batch_is(lib, ctx, s2, M[idx][::-1], "40 001 rows reversed")
    for x in (s2, s, b):
        x.close()


def test_column_sums_stripes_and_wide_sums(lib, ctx):
    """50 001 rows at k = 2 (no stripe count divides them) with columns whose sums pass 2^32."""
    n = 50001
    M = big_matrix(n, 16, seed=9, top_bits=21)
    M[:, 3] += 2 ** 20
    b = lib.Batch.from_counts(ctx, M)
    want = M.sum(axis=0)
    assert want[3] > 2 ** 35
    assert np.array_equal(b.column_sums(), want)
    assert_batch_is(lib, ctx, b, M, "50 001 x 16")
    b.close()


def test_gather_columns_past_one_pass_at_k3(lib, ctx, oracle):
    n, D = 16384 + 9, 64
    M = big_matrix(n, D, seed=11, top_bits=20)
    b = lib.Batch.from_counts(ctx, M)
    rng = np.random.default_rng(12)
    for table in (rng.permutation(D), rng.integers(0, D, D), np.full(D, D - 1)):
        g = b.gather_columns(table)
        assert_batch_is(lib, ctx, g, M[:, table], "16 393 x 64")
        g.close()
    b.close()


def test_gather_columns_one_wave_per_block_at_k7(lib, ctx):
    """At D = 16 384 a row fills the 64 KiB of LDS: one wave per block; 300 rows and arbitrary (non-permutation) tables."""
    n, D = 300, 16384
    rng = np.random.default_rng(13)
    M = rng.integers(0, 70000, (n, D))
    b = lib.Batch.from_counts(ctx, M)
    for table in (rng.permutation(D), rng.integers(0, D, D), np.arange(D)[::-1]):
        g = b.gather_columns(table)
        assert_batch_is(lib, ctx, g, M[:, table], "300 x 16 384")
        g.close()
    b.close()


@pytest.mark.parametrize("n,D", ((5003, 256), (70, 16384)))
def test_transform_kmers_host_arrays(n, D):
    """transform_kmers.transform_kmers on host arrays (phk_permute_columns_kernel) against NumPy fancy indexing."""
    from phamers_amd import transform_kmers as tk
    k = {256: 4, 16384: 7}[D]
    rng = np.random.default_rng(D)
    M = rng.integers(-2 ** 62, 2 ** 62, (n, D))
    for reverse, complement in ((True, False), (False, True), (True, True)):
        got = tk.transform_kmers(M, reverse=reverse, complement=complement, exact=True)
        assert got.dtype == M.dtype and np.array_equal(got, M[:, tk.exact_indices(k, reverse, complement)])
        if k == 4:
            got = tk.transform_kmers(M, reverse=reverse, complement=complement)
            assert np.array_equal(got, M[:, tk.reference_indices(k, reverse, complement)])


# ---- row sums of 2^32 and more ----------------------------------------------------------------------------------------
def test_row_sum_2_32_is_refused_not_wrapped(lib, ctx, oracle):
    """A batch keeps its row sums as uint32.  A row whose entries fit but whose sum is 2^32 or more must not come back with
    a wrapped sum (the scorers take it for T): phk_batch_from_counts refuses the matrix (Batch.from_counts -> None, the
    facade keeps the float rows), phk_batch_gather_columns refuses the table.  The last representable row, sum 2^32 - 1,
    normalises and scores like its float row."""
    with np.load(os.path.join(helpers.GOLDEN, "ref_features.npz")) as z:
        pos_c, neg_c = z["pos_counts"][:300].astype(np.int64), z["neg_counts"][:300].astype(np.int64)
        q_c = z["neg_counts"][300:303].astype(np.int64)
    D = 256
    big = q_c[0] * (U32 // int(q_c[0].sum()))
    big[int(np.argmax(big))] += U32 - int(big.sum())
    assert int(big.sum()) == U32
    last = np.stack([q_c[1], big, q_c[2]])
    b = lib.Batch.from_counts(ctx, last)
    assert b is not None
    assert np.array_equal(batch_rowsums(lib, ctx, b), np.array([q_c[1].sum(), U32, q_c[2].sum()], dtype=np.uint32))
    q = oracle.normalize_counts(last)
    assert_same_bits(b.normalized(), q, "row sum 2^32 - 1")
    pos, neg = oracle.normalize_counts(pos_c), oracle.normalize_counts(neg_c)
    cpos = np.stack([pos[i::10].mean(axis=0) for i in range(10)])
    cneg = np.stack([neg[i::10].mean(axis=0) for i in range(10)])
    model = lib.Model(ctx, pos, neg, cpos, cneg, k_neighbors=3)
    try:
        for method in ("knn", "kmeans", "combo"):
            want = oracle.score_points(q, pos, neg, method, 3, cpos, cneg)
            got, rows = b.score(model, method), model.score(q, method)
            # (the suite's standing bound of the float64 scores against the oracle, as in smoke(); the resident counts and
            # their float rows may take different kernels, so the two are held to the same bound against each other)
            assert helpers.rel_err(got, want) < 1e-6, method
            assert helpers.rel_err(rows, want) < 1e-6, method
            assert helpers.rel_err(got, rows) < 1e-6, method
    finally:
        model.close()
    # a gather that lifts a row's sum past 2^32: the constant table on the largest column of the large row
    with pytest.raises(lib.PhkError) as err:
        b.gather_columns(np.full(D, int(np.argmax(big))))
    assert err.value.code == lib.PHK_ERR_UNSUPPORTED
    g = b.gather_columns(np.arange(D)[::-1])        # (the batch and the context are fine afterwards)
    assert_batch_is(lib, ctx, g, last[:, ::-1], "after the refused gather")
    g.close()
    b.close()
    # sum exactly 2^32; the issue's [3e9, 3e9, 0, ..]; the overflowing row last of many
    over = last.copy()
    over[1, int(np.argmin(big))] += 1
    assert int(over[1].sum()) == 2 ** 32
    assert lib.Batch.from_counts(ctx, over) is None
    two = np.zeros((2, 16), dtype=np.int64)
    two[0, 3] = U32
    two[1, :2] = 3 * 10 ** 9
    assert lib.Batch.from_counts(ctx, two) is None
    ok = lib.Batch.from_counts(ctx, two[:1])
    assert ok is not None and batch_rowsums(lib, ctx, ok)[0] == U32
    ok.close()
    many = big_matrix(20001, 16, seed=3)
    many[-1, :] = 2 ** 28                              # 16 x 2^28 = 2^32
    assert lib.Batch.from_counts(ctx, many) is None
    many[-1, 0] -= 1
    b = lib.Batch.from_counts(ctx, many)
    assert b is not None and batch_rowsums(lib, ctx, b)[-1] == U32
    b.close()
