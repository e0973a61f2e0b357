"""Sliding-window counting on the path long sequences take (phamers_amd/csrc/windows.hip): rows DERIVED from their
predecessor -- added to at a leading cursor, subtracted from at a trailing one -- rather than counted in full.  A segment
of more than one window is forced with ``segment``, or reached by having more rows than the launch has walkers.  Every
batch is compared with tests/windows_ref.py, which counts every window on its own: the count matrix bit for bit, the
stored row sums (the kernels' running k-mer count, not a sum over the row), and the normalised rows with their empty
ones."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers, windows_ref

pytestmark = pytest.mark.gpu

BASES = np.array(list("ATGC"))


def rand_seq(rng, L, p=None):
    return "".join(BASES[rng.choice(4, L, p=p)]) if L else ""


def with_chars(seq, at, ch="N"):
    s = list(seq)
    for i in at:
        s[i] = ch
    return "".join(s)


def lowered(seq, a, b):
    return seq[:a] + seq[a:b].lower() + seq[b:]


def differences(batch, ref):
    """The names of what differs between a window batch and the reference: 'counts', 'row_sums', 'normalized'."""
    owner, _, want, sums = ref
    assert (batch.n, batch.D) == want.shape and batch.n == len(owner)
    bad = []
    got = batch.counts()
    assert got.dtype == np.int64
    if not np.array_equal(got, want):
        bad.append("counts (first at row %d)" % np.flatnonzero((got != want).any(axis=1))[0])
    stored = batch.row_sums()
    assert stored.dtype == np.uint32
    if not np.array_equal(stored.astype(np.int64), sums):
        bad.append("row_sums (first at row %d)" % np.flatnonzero(stored.astype(np.int64) != sums)[0])
    # kmer.normalize_counts of the rows: counts / row sum, a row without a counted k-mer NaN throughout
    norm = batch.normalized()
    assert norm.dtype == np.float64 and norm.shape == want.shape
    empty = sums == 0
    ok = np.array_equal(np.isnan(norm).all(axis=1), empty) and np.array_equal(np.isnan(norm).any(axis=1), empty)
    step = max(1, (1 << 22) // batch.D)
    for lo in range(0, batch.n if ok else 0, step):
        keep = ~empty[lo:lo + step]
        ok = ok and np.array_equal(norm[lo:lo + step][keep], want[lo:lo + step][keep] / sums[lo:lo + step][keep][:, None])
    if not ok:
        bad.append("normalized")
    return got, bad


def check(seqs, k, W, S, segment, ref=None):
    """The one road every case takes: Batch.windows_from_sequences against the reference.  Returns the count matrix."""
    from phamers_amd import _lib
    ref = ref if ref is not None else windows_ref.window_counts(seqs, k, W, S)
    batch = _lib.Batch.windows_from_sequences(_lib.get_context(), seqs, k, W, S, segment=segment)
    try:
        got, bad = differences(batch, ref)
    finally:
        batch.close()
    assert not bad, "k=%d W=%d S=%d segment=%d: %s differ from the reference" % (k, W, S, segment, ", ".join(bad))
    return got


def grid_pass(k):
    from phamers_amd import _lib
    n = ctypes.c_uint64()
    _lib.check(_lib.load().phk_windows_grid_pass(k, ctypes.byref(n)))
    return int(n.value)


# ---- a. derived rows at every k ----------------------------------------------------------------------------------------
AROUND_WORDS = (15, 16, 17, 31, 32, 33)     # around the 16-base packed word and the 32-base mask word


def every_k_seqs(k, invalid):
    rng = np.random.RandomState(300 + k)
    seqs = [rand_seq(rng, L) for L in (5, 63, 7, 64, 11, 300, 257)]
    if invalid:
        seqs[5] = lowered(with_chars(seqs[5], AROUND_WORDS), 120, 141)
        seqs[6] = lowered(with_chars(seqs[6], AROUND_WORDS), 200, 207)
    return seqs


@pytest.mark.parametrize("invalid", [False, True], ids=["clean", "invalid"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7])
def test_derived_rows_at_every_k(k, invalid):
    """W = 64, segments of 2 and 3 windows and one segment per sequence; the short sequences in front make the long ones
    start inside a packed word, and the invalid bases of the second variant sit around the word boundaries of those."""
    seqs = every_k_seqs(k, invalid)
    for S in (1, 5, 17):
        ref = windows_ref.window_counts(seqs, k, 64, S)
        assert ((ref[3] < 64 - k + 1).any() and (ref[3] == 64 - k + 1).any()) if invalid else (ref[3] == 64 - k + 1).all()
        for segment in (2, 3, 1000):
            check(seqs, k, 64, S, segment, ref)


# ---- b. an invalid base enters and leaves a window inside one segment ------------------------------------------------------
@pytest.mark.parametrize("S", [1, 10, 16])
@pytest.mark.parametrize("k", [4, 3, 7])
def test_invalid_bases_enter_and_leave_inside_one_segment(k, S):
    """One N at 200 and N at 300 .. 379 (longer than the window: all-zero rows in the middle of the segment, then
    recovery).  Every window wholly behind the last N must be the window of the sequence without any N: nothing of a
    k-mer that was masked on its way in, or on its way out, is left in the running histogram."""
    W = 50
    rng = np.random.RandomState(10 * k + S)
    clean = rand_seq(rng, 600)
    seq = with_chars(clean, [200] + list(range(300, 380)))
    ref = windows_ref.window_counts([seq], k, W, S)
    start, sums = ref[1], ref[3]
    assert (sums == 0).any() and sums[0] == W - k + 1 and sums[-1] == W - k + 1
    assert ((sums > 0) & (sums < W - k + 1)).any()
    got = check([seq], k, W, S, 1000, ref)
    behind = start >= 380
    assert behind.sum() >= 10
    assert np.array_equal(got[behind], windows_ref.window_counts([clean], k, W, S)[2][behind])


# ---- c. the step at which consecutive windows stop sharing k-mers ------------------------------------------------------
@pytest.mark.parametrize("invalid", [False, True], ids=["clean", "invalid"])
@pytest.mark.parametrize("k", [4, 3, 7])
def test_step_around_the_k_mers_of_a_window(k, invalid):
    """S = nk - 1 (the last step that derives: the cursors' ranges touch), nk and nk + 1 (every window counted in full),
    nk = W - k + 1."""
    W, nk = 40, 40 - k + 1
    rng = np.random.RandomState(50 + k)
    seqs = [rand_seq(rng, L) for L in (37, 40, 500, 9, 333)]
    if invalid:
        seqs[2] = lowered(with_chars(seqs[2], (0, 39, 40, 77, 250, 251, 499)), 300, 345)
        seqs[4] = with_chars(seqs[4], (36, 110, 332))
    for S in (nk - 1, nk, nk + 1):
        got = check(seqs, k, W, S, 4)
        assert got.shape[0] >= 20


# ---- d. cursor ranges of more than 64 packed words ---------------------------------------------------------------------
@pytest.mark.parametrize("invalid", [False, True], ids=["clean", "invalid"])
@pytest.mark.parametrize("W", [1100, 2500])
@pytest.mark.parametrize("k", [3, 5, 7, 4])
def test_cursor_ranges_longer_than_64_words(k, W, invalid):
    """The wave kernel (k != 4) takes 64 packed words = 1 024 bases per trip over a cursor's range.  S = 7: only the first
    window of a segment has a longer range; S = 1040 (still below nk): the leading and the trailing range of every derived
    row have.  k = 4: the lane kernel walks the same ranges word by word."""
    rng = np.random.RandomState(W + k)
    seqs = [rand_seq(rng, 6007), rand_seq(rng, 4100)]            # (6007: the second sequence starts inside a word)
    if invalid:
        for r in (0, 1):
            at = rng.choice(len(seqs[r]), 40, replace=False)
            seqs[r] = with_chars(seqs[r], at)
        seqs[1] = lowered(seqs[1], 2000, 2070)
    for S in (7, 1040):
        assert S < W - k + 1
        got = check(seqs, k, W, S, 3)
        assert got.shape[0] == (6007 - W) // S + 1 + (4100 - W) // S + 1


# ---- e. more segments than one pass of the grid, of mixed lengths ------------------------------------------------------
def short_sequences(rng, n, lengths, n_invalid):
    """n random sequences of the given lengths (drawn at random), a few of 0 and 15 bases in between, n_invalid N."""
    L = rng.choice(lengths, n)
    L[rng.choice(n, 6, replace=False)] = [0, 15, 0, 15, 15, 0]
    chars = BASES[rng.randint(0, 4, int(L.sum()))]
    chars[rng.choice(chars.shape[0], n_invalid, replace=False)] = "N"
    text = "".join(chars)
    cuts = np.concatenate(([0], np.cumsum(L)))
    return [text[cuts[i]:cuts[i + 1]] for i in range(n)]


@pytest.mark.parametrize("k", [4, 2, 5])
def test_grid_stride_with_derived_rows_of_mixed_segments(k):
    """W = 16, S = 1, segment = 3 on cap + 300 sequences of 16, 17 or 18 bases (cap = the segments one pass of the grid
    takes): every segment has 1, 2 or 3 windows, so in the k = 4 kernel the columns of finished segments stay as they are
    while their neighbours run on, and the second batch of a workgroup starts on that LDS.  About 82 000 rows at k = 4."""
    cap = grid_pass(k)
    assert 1024 <= cap <= 65536
    rng = np.random.RandomState(k)
    seqs = short_sequences(rng, cap + 300, (16, 17, 18), 12)
    ref = windows_ref.window_counts(seqs, k, 16, 1)
    per = np.bincount(ref[0], minlength=len(seqs))
    assert (per > 0).sum() > cap and set(per.tolist()) == {0, 1, 2, 3}      # more segments than one pass, of every length
    assert ref[2].shape[0] > cap and (ref[3] < 16 - k + 1).any()
    check(seqs, k, 16, 1, 3, ref)


def test_grid_stride_with_derived_rows_k7():
    """k = 7: one wave per workgroup.  cap + 60 sequences of 16 or 17 bases, W = 16: one or two windows each, about 3 100
    rows of 16 384 counts = 0.2 GB of rows on the device (0.4 GB as int64 on the host)."""
    cap = grid_pass(7)
    assert 1024 <= cap <= 4096
    rng = np.random.RandomState(7)
    seqs = short_sequences(rng, cap + 60, (16, 17), 8)
    ref = windows_ref.window_counts(seqs, 7, 16, 1)
    per = np.bincount(ref[0], minlength=len(seqs))
    assert (per > 0).sum() > cap and set(per.tolist()) == {0, 1, 2}
    assert ref[2].shape[0] > cap
    check(seqs, 7, 16, 1, 3, ref)


# ---- f. the segment the launch chooses when there are more rows than walkers ---------------------------------------------
@pytest.fixture(scope="module")
def compute_units():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked once in a child process: torch's HIP runtime has to
    be the first one initialised in its process, and this one has opened the device through libphamers_hip.so."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[-1])


@pytest.mark.parametrize("k", [3, 4])
def test_automatic_segment_above_one_window(compute_units, k):
    """segment = 0 with 2.5 times as many rows as the launch has walkers (128 per compute unit at k = 4, 16 at other k):
    the launch makes segments of three windows.  It does not report its choice, so the rows must also be those of
    segment = 1."""
    from phamers_amd import _lib
    assert 1 <= compute_units <= 1024
    walkers = compute_units * (128 if k == 4 else 16)
    W = 32
    rows = (5 * walkers + 1) // 2 + 100
    rng = np.random.RandomState(k)
    lengths = (rows // 2 + W - 1, rows - rows // 2 + W - 1)
    seqs = []
    for L in lengths:
        s = rand_seq(rng, L)
        seqs.append(with_chars(s, rng.choice(L, 25, replace=False)))
    ref = windows_ref.window_counts(seqs, k, W, 1)
    assert ref[2].shape[0] == rows >= 2.5 * walkers
    got = check(seqs, k, W, 1, 0, ref)
    batch = _lib.Batch.windows_from_sequences(_lib.get_context(), seqs, k, W, 1, segment=1)
    try:
        assert np.array_equal(batch.counts(), got) and np.array_equal(batch.row_sums().astype(np.int64), ref[3])
    finally:
        batch.close()


# ---- g. the last window ends on the last base of the stream --------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 1, 15, 16, 17, 31])
@pytest.mark.parametrize("k", [4, 7])
def test_last_window_ends_with_the_stream(k, tail):
    """T mod 32 = tail bases in the last mask word (and T mod 16 in the last packed word); one segment per sequence.
    Without an invalid base the kernels read no mask; with an N three bases before the end they do."""
    W, S = 40, 3
    last = W + 20 * S
    first = 41 + (tail - last - 41) % 32
    rng = np.random.RandomState(100 * k + tail)
    seqs = [rand_seq(rng, first), rand_seq(rng, last)]
    assert (first + last) % 32 == tail and (last - W) % S == 0
    ref = windows_ref.window_counts(seqs, k, W, S)
    assert ref[1][-1] + W == last
    check(seqs, k, W, S, 1000, ref)
    seqs[1] = with_chars(seqs[1], [last - 3])
    ref = windows_ref.window_counts(seqs, k, W, S)
    assert ref[3][-1] == W - k + 1 - min(k, 3)
    check(seqs, k, W, S, 1000, ref)


# ---- h. scores of derived rows -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scored():
    """Four sequences, one with 700 N, as windows of 600 every 150 in segments of 5 (derived rows, all-zero rows among
    them), and the same slices ingested as separate contigs; a reference of 600 + 600 rows with ten centroids each."""
    from phamers_amd import _lib, kmer
    f = helpers.load_npz("ref_features.npz")
    pos = kmer.normalize_counts(f["pos_counts"][:600].astype(np.int64))
    neg = kmer.normalize_counts(f["neg_counts"][:600].astype(np.int64))
    cpos = np.stack([pos[i::10].mean(axis=0) for i in range(10)])
    cneg = np.stack([neg[i::10].mean(axis=0) for i in range(10)])
    rng = np.random.RandomState(8)
    seqs = []
    for r, weights in enumerate(([0.35, 0.35, 0.15, 0.15], [0.15, 0.15, 0.35, 0.35], [0.25] * 4, [0.3, 0.2, 0.3, 0.2])):
        s = rand_seq(rng, 2000 + 53 * r, weights)
        seqs.append(with_chars(s, range(650, 1350)) if r == 2 else s)
    W, S = 600, 150
    ref = windows_ref.window_counts(seqs, 4, W, S)
    ctx = _lib.get_context()
    model = _lib.Model(ctx, pos, neg, cpos, cneg, k_neighbors=3)
    model.set_bandwidths(0.005, 0.01)
    windows = _lib.Batch.windows_from_sequences(ctx, seqs, 4, W, S, segment=5)
    empty = windows.row_sums() == 0
    chosen = windows.select(np.flatnonzero(~empty))
    contigs = _lib.Batch.from_sequences(ctx, [seqs[r][a:a + W] for r, a, z in zip(ref[0], ref[1], ref[3]) if z], 4)
    yield ref, model, empty, chosen, contigs
    for h in (windows, chosen, contigs, model):
        h.close()


@pytest.mark.parametrize("method", ["knn", "combo", "density"])
def test_scores_of_derived_rows_equal_scoring_the_slices(scored, method):
    ref, model, empty, chosen, contigs = scored
    assert np.array_equal(empty, ref[3] == 0) and empty.any() and not empty.all()
    assert np.array_equal(chosen.counts(), ref[2][~empty]) and np.array_equal(contigs.counts(), ref[2][~empty])
    got, want = chosen.score(model, method), contigs.score(model, method)
    assert got.shape == ((~empty).sum(),) and not np.isnan(want).any()
    assert np.array_equal(got, want)                 # the same rows through the same scorer: the same bits


# ---- i. the strand fold and the FASTA entry on derived rows ------------------------------------------------------------
def noisy_long_seqs(seed):
    rng = np.random.RandomState(seed)
    seqs = [rand_seq(rng, L) for L in (700, 64, 333, 50, 65)]
    seqs[0] = lowered(with_chars(seqs[0], (0, 63, 64, 300, 301, 699)), 400, 470)
    seqs[2] = with_chars(seqs[2], (100, 332))
    return seqs


@pytest.mark.parametrize("k", [4, 5])
def test_both_strands_of_derived_rows(k):
    from phamers_amd import kmer
    seqs = noisy_long_seqs(k)
    owner, start, want, sums = windows_ref.window_counts_folded(seqs, k, 64, 9)
    ids, got = kmer.count_windows(seqs, k, 64, 9, _segment=3, both_strands=True)
    assert ids == ["%d_%d" % (r, a) for r, a in zip(owner, start)]
    assert (sums == 0).any() and got.dtype == np.int64 and np.array_equal(got, want)


@pytest.mark.parametrize("k", [4, 3])
def test_fasta_entry_with_derived_rows(tmp_path, k):
    from phamers_amd import _lib
    seqs = noisy_long_seqs(20 + k)
    path = str(tmp_path / "w.fasta")
    with open(path, "w") as f:
        for r, s in enumerate(seqs):
            width = (60, 70, 33, 80, 16)[r]
            f.write(">rec%d some description\n" % r)
            f.write("\n".join(s[i:i + width] for i in range(0, len(s), width)) + "\n")
    ref = windows_ref.window_counts(seqs, k, 64, 9)
    by_strings = check(seqs, k, 64, 9, 3, ref)
    fasta = _lib.Fasta(path)
    try:
        batch = _lib.Batch.windows_from_fasta(_lib.get_context(), fasta, k, 64, 9, segment=3)
        try:
            got, bad = differences(batch, ref)
        finally:
            batch.close()
    finally:
        fasta.close()
    assert not bad, "k=%d from the file: %s differ from the reference" % (k, ", ".join(bad))
    assert np.array_equal(got, by_strings)
