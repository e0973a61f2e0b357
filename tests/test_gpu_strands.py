"""Strand-symmetric counting and scoring on the GPU (strands.hip, the both_strands options): integer results are compared
bit for bit with the CPU oracle's count of the sequence plus its count of the reverse complement, or with the NumPy fold
of tests/strands_ref.py; scores of a sequence and of its reverse complement must be the same bits."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import density_ref, helpers, strands_ref
from tests.helpers import REPO

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 4, 5, 6, 7]


def rand_seq(rng, L, alphabet="ATGC", p=None):
    return "".join(rng.choice(list(alphabet), L, p=p)) if L else ""


def both_strand_counts(seqs, k):
    """The oracle's count of every string plus its count of the string's reverse complement: (n, 4^k) int64."""
    from oracle import oracle
    rows = [np.asarray(oracle.count_string(s, k), dtype=np.int64) + np.asarray(oracle.count_string(strands_ref.revcomp(s), k), dtype=np.int64)
            for s in seqs]
    return np.array(rows, dtype=np.int64) if rows else np.zeros((0, 4 ** k), dtype=np.int64)


def grid_pass(k):
    from phamers_amd import _lib
    n = ctypes.c_uint64()
    _lib.check(_lib.load().phk_fold_grid_pass(k, ctypes.byref(n)))
    return int(n.value)


# ---- 1. every k ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_every_k_counts_both_strands(k):
    """Lengths 5 and 63 in front make the later sequences start in the middle of a packed word; N and lower case are
    invalid on both strands."""
    from phamers_amd import _lib, kmer
    rng = np.random.RandomState(40 + k)
    noisy = [0.235] * 4 + [0.02, 0.02, 0.02]
    seqs = [rand_seq(rng, L, "ATGCNat", noisy) for L in (5, 63, 0, k - 1, k, 64, 300)]
    want = both_strand_counts(seqs, k)
    assert want.sum() > 0 and (want.sum(axis=1) % 2 == 0).all()
    got = kmer.count(seqs, k, both_strands=True)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(kmer.count_string(seqs[-1], k, both_strands=True), want[-1])
    # the same batch, folded by hand: same rows, the stored row sums doubled
    batch = _lib.Batch.from_sequences(_lib.get_context(), seqs, k)
    try:
        forward, sums = batch.counts(), batch.row_sums()
        assert not batch.folded and np.array_equal(sums, forward.sum(axis=1))
        assert batch.fold_strands() is batch and batch.folded
        assert np.array_equal(batch.counts(), want)
        assert np.array_equal(batch.row_sums().astype(np.int64), 2 * sums.astype(np.int64))
        assert np.array_equal(batch.counts(), strands_ref.fold(forward))
    finally:
        batch.close()


def test_every_counting_entry_takes_the_option(tmp_path):
    from phamers_amd import kmer
    rng = np.random.RandomState(3)
    seqs = [rand_seq(rng, L, "ATGCN") for L in (700, 64, 333)]
    path = str(tmp_path / "s.fasta")
    with open(path, "w") as f:
        for r, s in enumerate(seqs):
            f.write(">SuperContig_%d_length_%d_ID_%d\n" % (r, len(s), r))
            f.write("\n".join(s[i:i + 61] for i in range(0, len(s), 61)) + "\n")
    want = both_strand_counts(seqs, 3)
    ids, got = kmer.count_file(path, 3, both_strands=True)
    assert len(ids) == 3 and np.array_equal(got, want)
    _, rows = kmer.count_directory(str(tmp_path), 3, identifier=".fasta", both_strands=True)
    assert np.array_equal(rows, want.sum(axis=0, keepdims=True).astype(float))
    cut_ids, cuts = kmer.count_cuts(seqs, 3, 100, both_strands=True)
    pieces = [s[a:a + 100] for s in seqs for a in range(0, len(s) - 99, 100)]
    assert len(cut_ids) == len(pieces) and np.array_equal(cuts, both_strand_counts(pieces, 3))
    rna = kmer.count(["AUGCCGUAAUG", "GGAUC"], 2, symbols=kmer.RNA, both_strands=True)
    assert np.array_equal(rna, both_strand_counts(["ATGCCGTAATG", "GGATC"], 2))
    # the default is the forward count, as before
    assert np.array_equal(kmer.count(seqs, 3), kmer.count(seqs, 3, both_strands=False))
    assert not np.array_equal(kmer.count(seqs, 3), want)


# ---- 2., 3. row counts around the kernel's grouping; the 64 KB row ---------------------------------------------------
def fold_random(k, n, seed, high=1000):
    from phamers_amd import _lib
    rng = np.random.RandomState(seed)
    counts = rng.randint(0, high, size=(n, 4 ** k)).astype(np.int64)      # every row differs
    batch = _lib.Batch.from_counts(_lib.get_context(), counts)
    try:
        batch.fold_strands()
        got, sums = batch.counts(), batch.row_sums()
    finally:
        batch.close()
    assert np.array_equal(got, strands_ref.fold(counts))
    assert np.array_equal(sums.astype(np.int64), 2 * counts.sum(axis=1))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("k", [4, 5])
def test_row_counts_around_a_workgroup(k, n):
    """A workgroup owns four rows at k <= 6 (one per wave): one to five rows."""
    assert grid_pass(k) % 4 == 0
    fold_random(k, n, 100 * k + n)


def test_more_rows_than_one_grid_pass():
    cap = grid_pass(4)
    assert 1024 <= cap <= 65536
    fold_random(4, cap + 5, 7)


@pytest.mark.parametrize("n", [1, 3])
def test_k7_row_fills_the_lds_of_a_workgroup(n):
    fold_random(7, n, 70 + n)


@pytest.mark.parametrize("k", [1, 2, 3, 6])
def test_other_k_from_random_counts(k):
    fold_random(k, 9, k)


# ---- 4. limits -------------------------------------------------------------------------------------------------------
def test_row_sum_limit():
    from oracle import oracle
    from phamers_amd import _lib
    ctx = _lib.get_context()
    rng = np.random.RandomState(1)
    counts = rng.randint(0, 50, size=(6, 256)).astype(np.int64)
    counts[2] = 0
    counts[2, [1, 6, 200]] = [2 ** 30, 2 ** 29, 5]
    counts[2, 0] = 2 ** 31 - 1 - counts[2].sum()
    assert counts[2].sum() == 2 ** 31 - 1 and counts[2, 0] >= 0
    batch = _lib.Batch.from_counts(ctx, counts)
    try:
        batch.fold_strands()
        assert np.array_equal(batch.counts(), strands_ref.fold(counts))
        assert int(batch.row_sums()[2]) == 2 ** 32 - 2
    finally:
        batch.close()
    # one row too many: refused before anything is written
    counts[4] = 0
    counts[4, 3] = 2 ** 31
    batch = _lib.Batch.from_counts(ctx, counts)
    try:
        with pytest.raises(_lib.PhkError) as e:
            batch.fold_strands()
        assert e.value.code == _lib.PHK_ERR_UNSUPPORTED and "1 row" in str(e.value)
        assert not batch.folded
        assert np.array_equal(batch.counts(), counts)
        assert np.array_equal(batch.row_sums().astype(np.int64), counts.sum(axis=1))
        # the batch still stands: it can be scored, and folded once the row is deselected
        ref = rng.randint(1, 50, size=(600, 256)).astype(np.float64)
        ref /= ref.sum(axis=1, keepdims=True)
        model = _lib.Model(ctx, ref[:300], ref[300:], k_neighbors=3)
        try:
            with ctx.options(force_exact=("1", "0")):          # (counts of 2^31 are far outside what the MFMA paths are tested for)
                got = batch.score(model, "knn")
        finally:
            model.close()
        assert np.array_equal(got, oracle.knn_score_points(oracle.normalize_counts(counts), ref[:300], ref[300:], 3))
        rest = batch.select([0, 1, 2, 3, 5])
        try:
            rest.fold_strands()
            assert np.array_equal(rest.counts(), strands_ref.fold(counts[[0, 1, 2, 3, 5]]))
        finally:
            rest.close()
    finally:
        batch.close()


def test_second_fold_empty_batch_and_inherited_mark():
    from phamers_amd import _lib, transform_kmers
    ctx = _lib.get_context()
    rng = np.random.RandomState(2)
    counts = rng.randint(0, 9, size=(5, 64)).astype(np.int64)
    batch = _lib.Batch.from_counts(ctx, counts)
    try:
        plain = batch.select([3, 1])
        assert not plain.folded
        plain.close()
        assert transform_kmers.fold_batch(batch) is batch
        once = batch.counts()
        with pytest.raises(_lib.PhkError) as e:
            batch.fold_strands()
        assert e.value.code == _lib.PHK_ERR_ARG
        assert np.array_equal(batch.counts(), once) and np.array_equal(batch.row_sums(), 2 * counts.sum(axis=1))
        sel = batch.select([4, 0])
        gat = batch.gather_columns(transform_kmers.exact_indices(3, True, True))
        try:
            assert sel.folded and gat.folded
            assert np.array_equal(sel.counts(), once[[4, 0]])
            assert np.array_equal(gat.counts(), once)                 # a folded row is its own reverse complement
            for b in (sel, gat):
                with pytest.raises(_lib.PhkError):
                    b.fold_strands()
        finally:
            sel.close()
            gat.close()
    finally:
        batch.close()
    empty = _lib.Batch.from_sequences(ctx, [], 4)
    try:
        assert empty.n == 0 and not empty.folded and empty.fold_strands().folded
    finally:
        empty.close()


# ---- 5. host entry ---------------------------------------------------------------------------------------------------
def test_host_matrix_fold():
    from phamers_amd import transform_kmers
    rng = np.random.RandomState(5)
    for k in (1, 3, 4, 5):
        counts = rng.randint(0, 2 ** 40, size=(7, 4 ** k), dtype=np.int64)
        got = transform_kmers.fold_strands(counts)
        assert got.dtype == np.int64 and np.array_equal(got, strands_ref.fold(counts))
    small = rng.randint(0, 100, size=(3, 16)).astype(np.uint16)
    assert np.array_equal(transform_kmers.fold_strands(small), strands_ref.fold(small))
    assert transform_kmers.fold_strands(np.zeros((0, 16), dtype=np.int64)).shape == (0, 16)
    with pytest.raises(TypeError):
        transform_kmers.fold_strands(counts.astype(float))
    with pytest.raises(ValueError):
        transform_kmers.fold_strands(np.ones((2, 100), dtype=np.int64))


# ---- 6. strand invariance --------------------------------------------------------------------------------------------
METHODS = ["knn", "kmeans", "combo", "density"]
K_CLUSTERS = 8


@pytest.fixture(scope="module")
def strands():
    """32 contigs of 600 bases (a few with an N) and their reverse complements; a folded reference of 64 + 64 rows from
    random sequences of two compositions.  The contigs are strand-asymmetric (purine-rich or pyrimidine-rich)."""
    from oracle import oracle
    rng = np.random.RandomState(17)
    mixes = ([0.4, 0.1, 0.4, 0.1], [0.1, 0.4, 0.1, 0.4], [0.35, 0.15, 0.3, 0.2], [0.3, 0.3, 0.2, 0.2])
    seqs = []
    for i in range(32):
        s = list(rand_seq(rng, 600, "ATGC", mixes[i % 4]))
        if i % 9 == 4:
            s[int(rng.randint(0, 600))] = "N"
        seqs.append("".join(s))
    rev = [strands_ref.revcomp(s) for s in seqs]
    pos_seqs = [rand_seq(rng, 600, "ATGC", [0.33, 0.27, 0.22, 0.18]) for _ in range(64)]
    neg_seqs = [rand_seq(rng, 600, "ATGC", [0.2, 0.22, 0.3, 0.28]) for _ in range(64)]
    pos_counts, neg_counts = oracle.count(pos_seqs, 4), oracle.count(neg_seqs, 4)
    pos = oracle.normalize_counts(strands_ref.fold(pos_counts))
    neg = oracle.normalize_counts(strands_ref.fold(neg_counts))
    q = oracle.normalize_counts(strands_ref.fold(oracle.count(seqs, 4)))
    forward = oracle.normalize_counts(pos_counts), oracle.normalize_counts(neg_counts)     # the same reference, not folded
    return seqs, rev, pos, neg, q, forward


@pytest.mark.parametrize("method", METHODS)
def test_scores_do_not_depend_on_the_strand(strands, method):
    from oracle import oracle
    from phamers_amd import learning, phamer
    seqs, rev, pos, neg, q, _ = strands
    fwd = phamer.score_contigs(seqs, pos, neg, method=method, both_strands=True, k_clusters=K_CLUSTERS)
    bwd = phamer.score_contigs(rev, pos, neg, method=method, both_strands=True, k_clusters=K_CLUSTERS)
    assert fwd.shape == (32,) and np.array_equal(fwd, bwd)
    if method == "density":
        want = density_ref.density_scores(q, pos, neg)
    else:
        # (the k-means fit is deterministic: these are the centroids the scorer fitted)
        cpos = learning.get_centroids(pos, learning.kmeans(pos, K_CLUSTERS))
        cneg = learning.get_centroids(neg, learning.kmeans(neg, K_CLUSTERS))
        want = oracle.score_points(q, pos, neg, method, 3, cpos, cneg)
    print("%s: rel err against the oracle %.3g" % (method, helpers.rel_err(fwd, want)))
    if method == "knn":
        assert np.array_equal(fwd, want)
    else:
        assert helpers.rel_err(fwd, want) < 1e-6


@pytest.mark.parametrize("method", METHODS)
def test_forward_counts_score_the_strands_differently(strands, method):
    """What the option buys: a forward-only run -- forward counts of the contigs against the same reference sequences
    counted forward -- scores the two strands of the same contigs differently (on the CPU oracle: 23 of the 32 under knn,
    all 32 under density, by up to 116).  Against the FOLDED reference forward counts of the two strands differ by rounding
    only: the reverse complement permutes the columns of the query, and a reference row that is its own permutation is
    equally far from both (the oracle: knn equal, density within 4e-13); that pair is printed, not asserted."""
    from phamers_amd import phamer
    seqs, rev, pos, neg, _, (pos_fwd, neg_fwd) = strands
    fwd = phamer.score_contigs(seqs, pos_fwd, neg_fwd, method=method, k_clusters=K_CLUSTERS)
    bwd = phamer.score_contigs(rev, pos_fwd, neg_fwd, method=method, both_strands=False, k_clusters=K_CLUSTERS)
    print("%s, forward reference: %d of 32 contigs score differently, by up to %.3g" % (
        method, int((fwd != bwd).sum()), float(np.abs(fwd - bwd).max())))
    assert (fwd != bwd).any()
    a = phamer.score_contigs(seqs, pos, neg, method=method, k_clusters=K_CLUSTERS)
    b = phamer.score_contigs(rev, pos, neg, method=method, k_clusters=K_CLUSTERS)
    print("%s, folded reference, forward queries: %d of 32 differ, by up to %.3g" % (
        method, int((a != b).sum()), float(np.abs(a - b).max())))


# ---- 7. windows ------------------------------------------------------------------------------------------------------
def test_window_counts_of_both_strands():
    from phamers_amd import kmer
    rng = np.random.RandomState(23)
    seqs = [rand_seq(rng, L, "ATGCNa", [0.24, 0.24, 0.24, 0.24, 0.02, 0.02]) for L in (7, 63, 50, 49, 333, 120)]
    ids, got = kmer.count_windows(seqs, 4, 50, 10, both_strands=True)
    sl = [(r, a, s[a:a + 50]) for r, s in enumerate(seqs) for a in range(0, len(s) - 50 + 1, 10)]
    assert ids == ["%d_%d" % (r, a) for r, a, _ in sl]
    assert np.array_equal(got, both_strand_counts([piece for _, _, piece in sl], 4))
    for k in (3, 5):
        _, got = kmer.count_windows(seqs, k, 50, 10, both_strands=True)
        assert np.array_equal(got, both_strand_counts([piece for _, _, piece in sl], k))


@pytest.mark.parametrize("method", ["combo", "density"])
def test_window_track_of_the_reverse_complement_is_the_track_reversed(method):
    from phamers_amd import kmer, transform_kmers, windows
    f = helpers.load_npz("ref_features.npz")
    pos = kmer.normalize_counts(transform_kmers.fold_strands(f["pos_counts"][:600].astype(np.int64)))
    neg = kmer.normalize_counts(transform_kmers.fold_strands(f["neg_counts"][:600].astype(np.int64)))
    rng = np.random.RandomState(29)
    W, S = 600, 150
    seqs = []
    for r, (L, mix) in enumerate(((W + 10 * S, [0.4, 0.1, 0.4, 0.1]), (W + 7 * S, [0.15, 0.35, 0.2, 0.3]), (W, [0.25] * 4))):
        s = list(rand_seq(rng, L, "ATGC", mix))
        if r == 0:
            s[500:1300] = "N" * 800                       # windows without a single valid k-mer: nan on both strands
        seqs.append("".join(s))
    track = windows.score_windows(seqs, pos, neg, window=W, step=S, method=method, k_clusters=12, both_strands=True)
    mirror = windows.score_windows([strands_ref.revcomp(s) for s in seqs], pos, neg, window=W, step=S, method=method,
                                   k_clusters=12, both_strands=True)
    assert len(track) == 11 + 8 + 1 and np.array_equal(track.owner, mirror.owner) and np.array_equal(track.start, mirror.start)
    assert np.isnan(track.scores).any() and not np.isnan(track.scores).all()
    for r in range(3):
        a, b = track.scores[track.owner == r], mirror.scores[mirror.owner == r][::-1]
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
    plain = windows.score_windows(seqs, pos, neg, window=W, step=S, method=method, k_clusters=12)
    assert not np.array_equal(plain.scores[~np.isnan(plain.scores)], track.scores[~np.isnan(track.scores)])


# ---- 8. the features cache holds forward counts ----------------------------------------------------------------------
def test_command_line_cache_rule(tmp_path):
    """`python -m phamers_amd.phamer ... --both_strands` three times in fresh child processes: from the FASTA file (the
    cache it writes holds FORWARD counts), again from that cache (the same phamer_scores.csv, byte for byte), and on the
    reverse-complemented FASTA file (the same score lines)."""
    from oracle import oracle
    from phamers_amd import fileIO, synth
    ref = helpers.load_npz("ref_features.npz")
    data = tmp_path / "data" / "reference_features"
    data.mkdir(parents=True)
    fileIO.save_counts(ref["pos_counts"], ref["pos_ids"], str(data / "positive_features.csv"))
    fileIO.save_counts(ref["neg_counts"], ref["neg_ids"], str(data / "negative_features.csv"))
    seqs = []
    for c in range(24):
        s = list(synth.synth_contig(5, c, 5000 + 13 * c))
        if c % 5 == 2:
            s[100 * c] = "N"
        seqs.append("".join(s))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE")}

    def run(name, sequences):
        indir = tmp_path / name
        if not indir.exists():
            indir.mkdir()
            with open(indir / "contigs.fasta", "w") as f:
                for c, s in enumerate(sequences):
                    f.write(">SuperContig_%d_length_%d_ID_%d\n" % (c, len(s), c))
                    f.write("\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + "\n")
        r = subprocess.run([sys.executable, "-m", "phamers_amd.phamer", "-in", str(indir), "-data", str(tmp_path / "data"), "-e",
                            "--both_strands"], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (name, r.stderr[-4000:])
        return (indir / "phamer_output" / "phamer_scores.csv").read_bytes(), indir / "contigs_features.csv"

    def lines(b):
        return b"\n".join(ln for ln in b.split(b"\n") if not ln.startswith(b"#"))
    cold, cache = run("fwd", seqs)
    assert b"both_strands" in cold and lines(cold).count(b"\n") >= 23
    _, cached = fileIO.read_feature_file(str(cache))
    assert np.array_equal(cached, oracle.count(seqs, 4))                        # forward counts, not folded ones
    warm, _ = run("fwd", seqs)                                                  # now starts from the cache
    assert warm == cold
    other, _ = run("rev", [strands_ref.revcomp(s) for s in seqs])
    assert lines(other) == lines(cold)
