"""Host check of tests/rows_ref.py: np_row_sum, the plain-Python statement of NumPy's summation order that the float
normalise kernel restates, equals np.sum bit for bit on every width tests/test_gpu_rows.py uses.  A NumPy that sums in
another order fails here first, before any device comparison is blamed on the kernel."""
import numpy as np
import pytest

from tests import rows_ref

ALL_WIDTHS = tuple(sorted(set(rows_ref.WIDTHS + rows_ref.POW4)))


def _bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


@pytest.mark.parametrize("D", ALL_WIDTHS)
def test_np_row_sum_is_np_sum(D):
    rows = rows_ref.float_rows(D, 12 if D <= 8192 else 40)
    for i in range(rows.shape[0]):
        want = np.sum(rows[i, :])            # a row of a 2-D matrix, as the reference's normalize_counts sums it
        assert _bits(rows_ref.np_row_sum(rows[i])) == _bits(want), (D, i)
        assert _bits(np.sum(rows[i].copy())) == _bits(want), (D, i)


@pytest.mark.parametrize("D", (1, 7, 8, 9, 129, 8193))
def test_np_row_sum_special_values(D):
    with np.errstate(invalid="ignore"):
        for row in rows_ref.float_special_rows(D):
            got, want = rows_ref.np_row_sum(row), np.sum(row)
            assert (np.isnan(got) and np.isnan(want)) or _bits(got) == _bits(want), (D, row[:4])


def test_the_float_rows_tell_the_two_orders_apart():
    """Above 8 192 columns (16 384 aside) pairwise summation of the whole row -- what the kernel did before it walked the
    row in pieces -- differs from np.sum on some of the very rows the device test uses: that test can see the difference."""
    for D in (8193, 12000, 16385, 20000, 65536):
        rows = rows_ref.float_rows(D, 40)
        differ = sum(rows_ref._pairwise(list(map(float, r)), 0, D) != np.sum(r) for r in rows)
        assert differ > 0, D
