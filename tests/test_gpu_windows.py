"""Sliding-window counts and scores on the GPU (windows.hip, kmer.count_windows, phamers_amd.windows): every row is compared
bit for bit with the oracle's count of the Python slice seq[a : a + W]."""
import ctypes

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu


def rand_seq(rng, L, alphabet="ATGC"):
    return "".join(rng.choice(list(alphabet), L)) if L else ""


def slices_of(seqs, W, S):
    return [(r, a, s[a:a + W]) for r, s in enumerate(seqs) for a in range(0, len(s) - W + 1, S)]


def want_counts(seqs, k, W, S):
    from oracle import oracle
    sl = slices_of(seqs, W, S)
    ids = ["%d_%d" % (r, a) for r, a, _ in sl]
    rows = [oracle.count_string(piece, k) for _, _, piece in sl]
    return ids, (np.array(rows, dtype=np.int64) if rows else np.zeros((0, 4 ** k), dtype=np.int64))


def check(seqs, k, W, S, segment=0):
    from phamers_amd import kmer
    ids, got = kmer.count_windows(seqs, k, W, S, _segment=segment)
    want_ids, want = want_counts(seqs, k, W, S)
    assert ids == want_ids
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("S", [1, 5, 32, 64, 100])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7])
def test_every_k(k, S):
    """W = 64; S = 64 and 100 share no k-mer between windows (every window is counted), the others slide.  The odd lengths
    in front make the later sequences start in the middle of a packed word (16 bases per word)."""
    rng = np.random.RandomState(100 * k + S)
    seqs = [rand_seq(rng, L) for L in (5, 63, 7, 64, 11, 300)]
    got = check(seqs, k, 64, S)
    assert got.shape[0] == 1 + (300 - 64) // S + 1 and (got.sum(axis=1) == 64 - k + 1).all()


@pytest.mark.parametrize("S", [1, 3, 16, 50])
@pytest.mark.parametrize("W", [4, 16, 17, 500])
def test_k4_lane_kernel(W, S):
    rng = np.random.RandomState(1000 * W + S)
    lengths = [0, 3, W - 1, W, W + 1, W + S - 1, W + S, W + S + 1, 2000] + list(rng.randint(0, 1500, 40))
    check([rand_seq(rng, int(L)) for L in lengths], 4, W, S)


W_INV, S_INV, A_INV = 50, 10, 100


@pytest.mark.parametrize("at", [A_INV - 1, A_INV, A_INV + W_INV - 4, A_INV + W_INV - 4 + 1, A_INV + W_INV - 1, A_INV + W_INV])
def test_one_invalid_base_around_a_window(at):
    """A single N just before / at the first base of the window at 100, at its last k-mer start and one past it, at its last
    base and one past it."""
    rng = np.random.RandomState(at)
    s = list(rand_seq(rng, 400))
    s[at] = "N"
    check(["".join(s)], 4, W_INV, S_INV)


def test_runs_of_invalid_bases_and_lower_case():
    rng = np.random.RandomState(7)
    s = rand_seq(rng, 400)
    gap = s[:130] + "N" * 60 + s[190:]
    got = check([gap], 4, W_INV, S_INV)
    assert (got.sum(axis=1) == 0).any()                        # windows inside the run: all-zero rows, written as zeros
    lower = s[:200] + s[200:260].lower() + s[260:]             # lower case is invalid under the reference's rule
    got = check([lower], 4, W_INV, S_INV)
    assert (got.sum(axis=1) == 0).any()
    for k in (3, 5):                                           # the wave-per-segment instances read the same mask
        check([gap, lower], k, W_INV, S_INV)


def grid_pass(k):
    from phamers_amd import _lib
    n = ctypes.c_uint64()
    _lib.check(_lib.load().phk_windows_grid_pass(k, ctypes.byref(n)))
    return int(n.value)


def test_segment_length_does_not_change_the_result():
    from phamers_amd import kmer
    rng = np.random.RandomState(11)
    seqs = [rand_seq(rng, 3000), rand_seq(rng, 3000)]
    want = check(seqs, 4, 100, 7, segment=0)
    for segment in (1, 2, 3, 64):
        assert np.array_equal(kmer.count_windows(seqs, 4, 100, 7, _segment=segment)[1], want)
    for k in (3, 6):
        base = check(seqs, k, 100, 7, segment=0)
        for segment in (1, 3, 64):
            assert np.array_equal(kmer.count_windows(seqs, k, 100, 7, _segment=segment)[1], base)


@pytest.mark.parametrize("k", [2, 4])
def test_more_segments_than_one_grid_pass(k):
    """One window per segment and more windows than the launch takes in a single pass of its grid (the launch code's own
    figure): the kernels' grid-stride loops run."""
    cap = grid_pass(k)
    assert 1024 <= cap <= 65536
    rng = np.random.RandomState(k)
    W = 16
    seqs = [rand_seq(rng, 37), rand_seq(rng, cap + 200 + W - 1)]
    got = check(seqs, k, W, 1, segment=1)
    assert got.shape[0] == 37 - W + 1 + cap + 200 > cap


def test_windows_with_step_equal_to_window_are_the_cuts():
    from phamers_amd import kmer
    rng = np.random.RandomState(5)
    seqs = [rand_seq(rng, int(L), "ATGCN") for L in (0, 99, 100, 101, 1234, 777)]
    ids, got = kmer.count_windows(seqs, 4, 100, 100)
    cut_ids, cuts = kmer.count_cuts(seqs, 4, 100)
    assert np.array_equal(got, cuts) and len(ids) == len(cut_ids)
    assert ids[:2] == ["2_0", "3_0"] and ids[2:4] == ["4_0", "4_100"]   # (starts, where count_cuts numbers its pieces)


def test_counts_beyond_16_bits():
    from phamers_amd import kmer
    ids, got = kmer.count_windows(["A" * 140000], 4, 70000, 35000)
    assert ids == ["0_0", "0_35000", "0_70000"]
    want = np.zeros((3, 256), dtype=np.int64)
    want[:, 0] = 69997
    assert np.array_equal(got, want)


def test_fasta_path(tmp_path):
    from phamers_amd import kmer
    rng = np.random.RandomState(3)
    seqs = [rand_seq(rng, L, "ATGCN") for L in (700, 64, 333, 50)]
    path = str(tmp_path / "w.fasta")
    with open(path, "w") as f:
        for r, s in enumerate(seqs):
            width = (60, 70, 33, 80)[r]
            f.write(">rec%d some description\n" % r)
            f.write("\n".join(s[i:i + width] for i in range(0, len(s), width)) + "\n")
    ids, got = kmer.count_windows(path, 4, 64, 9)
    _, by_strings = kmer.count_windows(seqs, 4, 64, 9)
    want_ids, want = want_counts(seqs, 4, 64, 9)
    assert np.array_equal(got, by_strings) and np.array_equal(got, want)
    assert ids == ["rec" + i for i in want_ids]                       # line breaks do not shift the starts
    assert ids[0] == "rec0_0" and ids[1] == "rec0_9" and "rec3_0" not in ids and ids[-1] == "rec2_261"


@pytest.fixture(scope="module")
def reference():
    from phamers_amd import kmer
    f = helpers.load_npz("ref_features.npz")
    pos = kmer.normalize_counts(f["pos_counts"][:600].astype(np.int64))
    neg = kmer.normalize_counts(f["neg_counts"][:600].astype(np.int64))
    rng = np.random.RandomState(8)
    seqs = []
    for r, weights in enumerate(([0.35, 0.35, 0.15, 0.15], [0.15, 0.15, 0.35, 0.35], [0.25] * 4, [0.3, 0.2, 0.3, 0.2])):
        s = list(rng.choice(list("ATGC"), 2000 + 53 * r, p=weights))
        if r == 2:
            s[650:1350] = "N" * 700
        seqs.append("".join(s))
    return pos, neg, seqs


@pytest.mark.parametrize("method", ["knn", "kmeans", "combo", "density"])
def test_scores_equal_scoring_the_slices_as_contigs(reference, method):
    from phamers_amd import _lib, windows
    from oracle import oracle
    pos, neg, seqs = reference
    W, S = 600, 150
    track = windows.score_windows(seqs, pos, neg, window=W, step=S, method=method, k_clusters=12)
    sl = slices_of(seqs, W, S)
    assert track.record_ids == ["0", "1", "2", "3"] and track.window == W
    assert track.owner.tolist() == [r for r, _, _ in sl] and track.start.tolist() == [a for _, a, _ in sl]
    empty = np.array([oracle.count_string(piece, 4).sum() == 0 for _, _, piece in sl])
    assert empty.any() and track.scores.dtype == np.float64
    assert np.array_equal(np.isnan(track.scores), empty)
    # the existing path: a model with the same centroids, queried with the counts of the slices as separate contigs
    ctx = _lib.get_context()
    with_centroids = method in ("kmeans", "combo")
    assert (track.positive_centroids is not None) == with_centroids
    model = _lib.Model(ctx, pos, neg, track.positive_centroids if with_centroids else None,
                       track.negative_centroids if with_centroids else None, k_neighbors=3)
    try:
        if method == "density":
            model.set_bandwidths(0.005, 0.01)
        batch = _lib.Batch.from_sequences(ctx, [piece for (_, _, piece), e in zip(sl, empty) if not e], 4)
        try:
            want = batch.score(model, method)
        finally:
            batch.close()
    finally:
        model.close()
    assert np.array_equal(track.scores[~empty], want)
    regions = windows.call_regions(track, threshold=float(np.nanmedian(track.scores)))
    assert regions and all(r[3] >= 1 and r[2] - r[1] == W + (r[3] - 1) * S for r in regions)


def test_errors():
    from phamers_amd import _lib, kmer
    with pytest.raises(ValueError):
        kmer.count_windows(["ACGT" * 10], 4, 3, 1)
    with pytest.raises(ValueError):
        kmer.count_windows(["ACGT" * 10], 4, 8, 0)
    ids, none = kmer.count_windows(["ACGT"], 4, 8, 1)               # no window: no row, and no call into the library
    assert ids == [] and none.shape == (0, 256) and none.dtype == np.int64
    ctx = _lib.get_context()
    bases = np.frombuffer(b"ACGTACGTACGT", dtype=np.uint8)
    off = np.array([0, 12], dtype=np.uint64)

    def call(k, window, step, offsets=off, out=True):
        h = ctypes.c_void_p()
        rc = ctx.lib.phk_batch_windows_from_ascii(ctx.handle, _lib.ptr(bases), None if offsets is None else _lib.ptr(offsets), 1, k,
                                                  b"ATGC", window, step, 0, ctypes.byref(h) if out else None)
        if rc == 0:
            ctx.lib.phk_batch_free(ctx.handle, h)
        return rc
    assert call(4, 3, 1) == -1 and call(4, 8, 0) == -1            # PHK_ERR_ARG: window < k, step < 1
    assert call(4, 8, 1, offsets=None) == -1 and call(4, 8, 1, out=False) == -1
    assert call(4, 13, 1) == -1                                   # no window at all
    assert call(8, 8, 1) == -4                                    # PHK_ERR_UNSUPPORTED: k > PHK_MAX_K
    assert call(4, 8, 1) == 0
    # the batch stands as any other: shape, normalised rows, selection
    b = _lib.Batch.windows_from_sequences(ctx, ["ACGTACGTACGT"], 4, 8, 2)
    try:
        assert (b.n, b.D, b.total_bases, b.any_invalid) == (3, 256, 24, False)
        assert b.row_sums().tolist() == [5, 5, 5]
        assert np.array_equal(b.normalized(), b.counts() / 5.0)
        s = b.select([2, 0])
        assert np.array_equal(s.counts(), b.counts()[[2, 0]])
        s.close()
    finally:
        b.close()
