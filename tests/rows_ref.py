"""NumPy's summation order for a contiguous float64 row, in plain Python floats: the reference statement of what
phk_normalize_f64_kernel (phamers_amd/csrc/rows.hip) has to reproduce.  Test-only code.

np.sum hands its reduction loop at most np.getbufsize() = 8 192 elements at a time.  Each piece is summed pairwise:
blocks of at most 128 elements with eight running partial sums, larger pieces halved with the split rounded down to a
multiple of 8.  The pieces' sums are added one after another to a result that starts at +0.0.
tests/test_rows_host.py pins this to np.sum itself; a NumPy that sums in another order fails there first."""

BUFSIZE = 8192
BLOCK = 128


def _leaf(a, lo, n):
    if n < 8:
        r = 0.0
        for i in range(lo, lo + n):
            r += a[i]
        return r
    r0, r1, r2, r3, r4, r5, r6, r7 = a[lo:lo + 8]
    end = lo + n - n % 8
    for i in range(lo + 8, end, 8):
        r0 += a[i]
        r1 += a[i + 1]
        r2 += a[i + 2]
        r3 += a[i + 3]
        r4 += a[i + 4]
        r5 += a[i + 5]
        r6 += a[i + 6]
        r7 += a[i + 7]
    res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7))
    for i in range(end, lo + n):
        res += a[i]
    return res


def _pairwise(a, lo, n):
    if n <= BLOCK:
        return _leaf(a, lo, n)
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a, lo, n2) + _pairwise(a, lo + n2, n - n2)


def np_row_sum(a):
    """np.sum of a 1-D float64 row, as a Python float."""
    a = [float(x) for x in a]
    s = 0.0
    for lo in range(0, len(a), BUFSIZE):
        s = s + _pairwise(a, lo, min(BUFSIZE, len(a) - lo))
    return s


# the widths of the host entry points' tests (every 4^k is added by the callers)
WIDTHS = (1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 130, 136, 137, 255, 257, 1000, 8191, 8192, 8193, 12000, 16385, 20000,
          65536)
POW4 = tuple(4 ** k for k in range(1, 8))


# ---- inputs shared by the host and the device tests -------------------------------------------------------------------
def float_rows(D, n, seed=0):
    """n rows of D float64 values with magnitudes mixed over six decades (the same rows for the same (D, n, seed))."""
    import numpy as np
    rng = np.random.default_rng([seed, D, n])
    return rng.random((n, D)) * rng.choice([1.0, 1e3, 1e-3], (n, D))


def float_special_rows(D):
    """Rows of D float64 values holding -0.0, a zero sum with and without entries, and an inf."""
    import numpy as np
    rng = np.random.default_rng([7, D])
    a = rng.random((6, D)) + 0.5
    a[0, ::2] = -0.0                   # -0.0 among ordinary values
    a[1, :] = -0.0                     # nothing but -0.0: sum 0, every entry NaN
    a[2, :] = 0.0                      # zero row
    a[3, :] = 0.0
    if D > 1:
        a[3, 0], a[3, D - 1] = 1.5, -1.5   # sums to zero with entries: +inf, -inf, NaN elsewhere
    a[4, D // 2] = np.inf              # inf / inf = NaN, the rest 0
    return a                           # (row 5 stays ordinary: the neighbours of odd rows must come out untouched)


SMALL_PRIMES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 97, 251, 257, 4999, 65537, 2147483647)


def row_with_sum(rng, D, S, cap):
    """D non-negative integers, none above cap, that sum to exactly S (Python-int arithmetic for the remainder)."""
    import numpy as np
    assert 0 <= S <= D * cap
    w = rng.random(D) + 1e-3
    e = np.minimum(np.floor(w / w.sum() * (S * (1.0 - 1e-6))), float(min(cap, 2 ** 62))).astype(np.int64)
    rem = int(S) - int(e.sum())
    assert rem >= 0
    for j in rng.permutation(D):
        if rem == 0:
            break
        add = min(rem, int(cap) - int(e[j]))
        if rem > 64 and add == rem and D > 1:
            add = rem - rem // 3       # (leave something for the next entries as well)
        e[j] += add
        rem -= add
    if rem:
        for j in range(D):
            add = min(rem, int(cap) - int(e[j]))
            e[j] += add
            rem -= add
    assert rem == 0 and int(e.sum()) == S and int(e.max()) <= cap and int(e.min()) >= 0
    return e


def division_rows(D, mmax, cap, max_sum=None, seed=0, every=1):
    """An int64 matrix aimed at the division: rows whose sums are exactly 2^m - 1, 2^m, 2^m + 1 (m <= mmax) and small
    primes, as far as D entries of at most cap (and a row sum of at most max_sum) can hold them; a row with the single
    non-zero entry min(cap, 2^32 - 1); a row of nothing but 2^32 - 1 where the bounds allow it; all-zero rows second, inside
    and last.  `every` thins the targets out for very wide rows."""
    import numpy as np
    rng = np.random.default_rng([seed, D, mmax])
    top = D * cap if max_sum is None else min(D * cap, max_sum)
    targets = list(SMALL_PRIMES)
    for m in range(1, mmax + 1):
        targets += [2 ** m - 1, 2 ** m, 2 ** m + 1]
    targets = [S for S in sorted(set(targets)) if 1 <= S <= top][::every]
    rows = [row_with_sum(rng, D, S, cap) for S in targets]
    single = np.zeros(D, dtype=np.int64)
    single[D // 3] = min(cap, 2 ** 32 - 1)
    rows.append(single)
    if cap >= 2 ** 32 - 1 and D * (2 ** 32 - 1) <= top:
        rows.append(np.full(D, 2 ** 32 - 1, dtype=np.int64))
    zero = np.zeros(D, dtype=np.int64)
    half = len(rows) // 2
    rows = rows[:1] + [zero] + rows[1:half] + [zero, zero] + rows[half:] + [zero]
    return np.stack(rows)
