"""NumPy restatement of sliding-window k-mer counting, for the tests: every window is counted on
its own from the per-base codes -- the k-mer code and the validity of every k-mer start are computed once, then the
(window, code) pairs of every window are scattered with one bincount.  No row is derived from another, so nothing here
resembles the add / subtract scheme of phamers_amd/csrc/windows.hip.  Invalid characters follow oracle.count_string:
whatever is not (case-sensitively) one of the four symbols is invalid, and a k-mer that holds one is not counted.
tests/test_windows_host.py pins this to the oracle row by row.  Test-only code."""
import numpy as np

from tests import strands_ref

CHUNK = 1 << 22   # (window, k-mer start) pairs and histogram cells per bincount, at most (bounds the temporaries)


def base_codes(seq, symbols="ATGC"):
    """int8 per character: the index of the character in ``symbols``, -1 for anything else."""
    lut = np.full(256, -1, dtype=np.int8)
    for i, ch in enumerate(symbols):
        lut[ord(ch)] = i
    return lut[np.frombuffer(seq.encode("latin-1", "replace"), dtype=np.uint8)]


def kmer_starts(codes, k):
    """(code int64, valid bool) of the k-mer starting at every position of ``codes`` (first base most significant); the
    last k - 1 positions, where no k-mer fits, are invalid."""
    T = codes.shape[0]
    n = max(T - k + 1, 0)
    code = np.zeros(T, dtype=np.int64)
    valid = np.zeros(T, dtype=bool)
    valid[:n] = True
    for j in range(k):
        c = codes[j:j + n].astype(np.int64)
        valid[:n] &= c >= 0
        code[:n] = code[:n] * 4 + np.where(c >= 0, c, 0)
    return code, valid


def count_at(codes, first, k, nk):
    """Row i = the histogram of the valid k-mers starting at first[i] .. first[i] + nk - 1 of the code stream:
    (counts int64 (rows, 4^k), sums int64 (rows,)).  The sums count the valid starts; they are not added up from counts."""
    D = 4 ** k
    rows = first.shape[0]
    counts = np.zeros((rows, D), dtype=np.int64)
    sums = np.zeros(rows, dtype=np.int64)
    code, valid = kmer_starts(codes, k)
    step = max(1, CHUNK // max(nk, D))
    span = np.arange(nk, dtype=np.int64)
    for lo in range(0, rows, step):
        hi = min(rows, lo + step)
        at = first[lo:hi, None] + span[None, :]                        # (windows, nk) k-mer starts
        ok = valid[at]
        cell = (np.arange(hi - lo, dtype=np.int64)[:, None] * D + code[at])[ok]
        counts[lo:hi] = np.bincount(cell, minlength=(hi - lo) * D).reshape(hi - lo, D)
        sums[lo:hi] = ok.sum(axis=1)
    return counts, sums


def plan(lengths, W, S):
    """(owner, start) of every window in row order: sequence-major, starts 0, S, 2 S, ... while start + W <= length."""
    owner, start = [], []
    for r, L in enumerate(lengths):
        a = np.arange(0, L - W + 1, S, dtype=np.int64) if L >= W else np.zeros(0, dtype=np.int64)
        owner.append(np.full(a.shape[0], r, dtype=np.int64))
        start.append(a)
    if not owner:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(owner), np.concatenate(start)


def _stream(seqs, symbols):
    lengths = np.array([len(s) for s in seqs], dtype=np.int64)
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    codes = base_codes("".join(seqs), symbols)
    assert codes.shape[0] == offsets[-1]
    return lengths, offsets, codes


def window_counts(seqs, k, W, S, symbols="ATGC"):
    """(owner, start, counts int64 (rows, 4^k), sums int64 (rows,)): row i is the k-mer count of
    seqs[owner[i]][start[i] : start[i] + W], sums[i] its number of counted k-mers."""
    k, W, S = int(k), int(W), int(S)
    assert 1 <= k <= W and S >= 1
    lengths, offsets, codes = _stream(seqs, symbols)
    owner, start = plan(lengths, W, S)
    # (a window lies inside its sequence, so none of its W - k + 1 k-mers reaches into the next one)
    counts, sums = count_at(codes, offsets[owner] + start, k, W - k + 1)
    return owner, start, counts, sums


def window_counts_folded(seqs, k, W, S, symbols="ATGC"):
    """Both strands: every window's count plus the count of the window's reverse complement.  The reverse complement of
    s[a : a + W] is the slice [L - a - W, L - a) of the reverse complement of s, counted there like any window."""
    k, W, S = int(k), int(W), int(S)
    assert 1 <= k <= W and S >= 1 and symbols == "ATGC"
    owner, start, counts, sums = window_counts(seqs, k, W, S, symbols)
    lengths, offsets, codes = _stream([strands_ref.revcomp(s) for s in seqs], symbols)
    back, back_sums = count_at(codes, offsets[owner] + lengths[owner] - start - W, k, W - k + 1)
    return owner, start, counts + back, sums + back_sums
