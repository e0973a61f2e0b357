"""NumPy restatement of the strand fold, for the tests: the column of the reverse-complement k-mer
from the base-4 digits, the fold of a count matrix, the reverse complement of a string.  Test-only code."""
import numpy as np

COMPLEMENT = {"A": "T", "T": "A", "G": "C", "C": "G"}


def rc_table(k):
    """rc[c] = the column of the reverse complement of k-mer c.  Digit order A=0, T=1, G=2, C=3, first base most
    significant: reverse the k digits, flip bit 0 of each."""
    table = np.zeros(4 ** k, dtype=np.int64)
    for c in range(4 ** k):
        digits = [(c >> (2 * (k - 1 - i))) & 3 for i in range(k)]       # first base first
        out = 0
        for d in reversed(digits):
            out = out * 4 + (d ^ 1)
        table[c] = out
    return table


def fold(counts):
    """counts + counts[..., rc]: a row (4^k,) or a matrix (n, 4^k), int64."""
    counts = np.asarray(counts, dtype=np.int64)
    D = counts.shape[-1]
    k = int(round(np.log(D) / np.log(4)))
    assert 4 ** k == D
    return counts + counts[..., rc_table(k)]


def revcomp(s):
    """A<->T, G<->C, every other character as it is, order reversed."""
    return "".join(COMPLEMENT.get(ch, ch) for ch in reversed(s))
