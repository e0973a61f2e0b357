"""CPU-only: the window plan, region calling, the track file and the command line of phamers_amd.windows; the reference of
the GPU window tests (tests/windows_ref.py) against the oracle."""
import argparse
import os

import numpy as np
import pytest

from tests.helpers import REPO


def plan_by_loops(lengths, W, S):
    owner, start = [], []
    for r, L in enumerate(lengths):
        j = 0
        while j * S + W <= L:
            owner.append(r)
            start.append(j * S)
            j += 1
    return np.array(owner, dtype=np.int64), np.array(start, dtype=np.int64)


@pytest.mark.parametrize("W,S", [(8, 1), (8, 3), (8, 8), (8, 11), (10, 5)])
def test_window_plan_equals_a_double_loop(W, S):
    from phamers_amd import kmer
    lengths = [0, 1, W - 1, W, W + 1, W + S - 1, W + S, 3 * W + 7]
    owner, start = kmer.window_plan(lengths, W, S)
    want_owner, want_start = plan_by_loops(lengths, W, S)
    assert owner.dtype == np.int64 and start.dtype == np.int64
    assert np.array_equal(owner, want_owner) and np.array_equal(start, want_start)
    # (L - W) // S + 1 windows per sequence that is long enough
    assert [int((owner == r).sum()) for r in range(len(lengths))] == [(L - W) // S + 1 if L >= W else 0 for L in lengths]


def test_window_plan_of_nothing():
    from phamers_amd import kmer
    owner, start = kmer.window_plan([], 8, 2)
    assert owner.shape == (0,) and start.shape == (0,)
    owner, start = kmer.window_plan([3, 7], 8, 2)
    assert owner.shape == (0,) and start.shape == (0,)


def test_count_windows_refuses_bad_window_and_step_before_any_device_work(monkeypatch):
    from phamers_amd import _lib, kmer

    def no_device(*a, **kw):
        raise AssertionError("the arguments are checked before a context is asked for")
    monkeypatch.setattr(_lib, "get_context", no_device)
    with pytest.raises(ValueError):
        kmer.count_windows(["ACGTACGT"], 4, 3, 1)          # window < kmer_length
    with pytest.raises(ValueError):
        kmer.count_windows(["ACGTACGT"], 4, 8, 0)          # step < 1
    with pytest.raises(ValueError):
        kmer.window_plan([10], 8, 0)


def track_of(owner, scores, window=100, step=10, records=("a", "b", "c")):
    from phamers_amd import windows
    owner = np.asarray(owner)
    start = np.zeros(len(owner), dtype=np.int64)
    for r in set(owner.tolist()):
        start[owner == r] = np.arange((owner == r).sum()) * step
    return windows.WindowTrack(list(records), owner, start, window, step, np.asarray(scores, dtype=float))


def test_call_regions_on_hand_written_tracks():
    from phamers_amd import windows
    nan = float("nan")
    # a run broken by NaN
    t = track_of([0] * 6, [1.0, 2.0, nan, 3.0, 0.5, -1.0])
    assert windows.call_regions(t) == [("a", 0, 110, 2, 1.5, 2.0), ("a", 30, 140, 2, 1.75, 3.0)]
    # a run broken by a record boundary, and one ending at the last window
    t = track_of([0, 0, 0, 1, 1, 1], [-1.0, 1.0, 1.0, 1.0, -1.0, 4.0])
    assert windows.call_regions(t) == [("a", 10, 120, 2, 1.0, 1.0), ("b", 0, 100, 1, 1.0, 1.0), ("b", 20, 120, 1, 4.0, 4.0)]
    # min_windows = 2 drops the single hits
    assert windows.call_regions(t, min_windows=2) == [("a", 10, 120, 2, 1.0, 1.0)]
    # a score equal to the threshold is no hit
    t = track_of([0, 0, 0, 0], [0.5, 0.5000001, 0.5, 0.4])
    assert windows.call_regions(t, threshold=0.5) == [("a", 10, 110, 1, 0.5000001, 0.5000001)]
    assert windows.call_regions(t, threshold=0.0) == [("a", 0, 130, 4, float(np.mean([0.5, 0.5000001, 0.5, 0.4])), 0.5000001)]
    # nothing above, all NaN, no window at all
    assert windows.call_regions(track_of([0, 1], [-1.0, -2.0])) == []
    assert windows.call_regions(track_of([0, 1], [nan, nan])) == []
    assert windows.call_regions(track_of([], [])) == []
    # records without windows in between do not join their neighbours
    t = track_of([0, 2], [1.0, 1.0])
    assert windows.call_regions(t) == [("a", 0, 100, 1, 1.0, 1.0), ("c", 0, 100, 1, 1.0, 1.0)]


def test_save_track_and_regions_read_back(tmp_path):
    from phamers_amd import fileIO, windows
    t = track_of([0, 0, 1], [0.1 + 0.2, float("nan"), -3.5e-7], records=("rec,with comma", "b"))
    args = argparse.Namespace(window=100, step=10)
    path = str(tmp_path / "window_scores.csv")
    windows.save_track(path, t, args=args)
    text = open(path).read()
    assert text.startswith("# " + fileIO.generate_summary(args, header="PhaMers window score file").split("\n")[0] + "\n")
    assert "# window:\t100\n" in text and "# step:\t10\n" in text and "# record_id,start,end,score\n" in text
    ids, start, end, scores = windows.read_track(path)
    assert ids == ["rec,with comma", "rec,with comma", "b"]
    assert np.array_equal(start, t.start) and np.array_equal(end, t.start + 100)
    assert np.array_equal(scores, t.scores, equal_nan=True)              # repr(float) round-trips bit for bit
    rpath = str(tmp_path / "phage_regions.csv")
    regions = windows.call_regions(t)
    windows.save_regions(rpath, regions)
    body = [line for line in open(rpath).read().split("\n") if line and not line.startswith("#")]
    assert body == ["rec,with comma,0,100,1,%r,%r" % (0.1 + 0.2, 0.1 + 0.2)]


def test_command_line_parses():
    from phamers_amd import windows
    a = windows._parser().parse_args(["-in", "g.fasta", "-out", "o"])
    assert (a.fasta_file, a.output_directory, a.window, a.step, a.kmer_length, a.method, a.threshold, a.min_windows) == \
        ("g.fasta", "o", 5000, 500, 4, "combo", 0.0, 1)
    a = windows._parser().parse_args("-in g.fa -out o -w 600 -s 150 -k 5 -m knn -t 0.25 -min 3 -pf p.csv -nf n.csv".split())
    assert (a.window, a.step, a.kmer_length, a.method, a.threshold, a.min_windows) == (600, 150, 5, "knn", 0.25, 3)
    assert (a.positive_features, a.negative_features, a.data_directory) == ("p.csv", "n.csv", None)
    with pytest.raises(SystemExit):
        windows._parser().parse_args(["-out", "o"])


def test_windows_module_does_not_import_oracle():
    text = open(os.path.join(REPO, "phamers_amd", "windows.py")).read()
    assert "import oracle" not in text and "from oracle" not in text


# ---- tests/windows_ref.py, the reference of the GPU window tests, against the oracle -----------------------------------
def noisy_seqs(seed, W):
    """Lengths below, at and above W, around it and in the middle of a packed word; N and lower case (both invalid)."""
    rng = np.random.RandomState(seed)
    alphabet, p = list("ATGCNatgc"), [0.22] * 4 + [0.04] + [0.02] * 4
    lengths = (0, 5, W - 1, W, W + 1, 63, 2 * W + 3, 300)
    seqs = ["".join(rng.choice(alphabet, L, p=p)) if L else "" for L in lengths]
    s = list(seqs[-1])
    s[100:100 + W + 5] = "N" * (W + 5)             # windows without a single valid k-mer
    s[200:230] = "".join(s[200:230]).lower()
    seqs[-1] = "".join(s)
    return seqs


@pytest.mark.parametrize("W,S", [(24, 1), (24, 7), (24, 24), (24, 31), (7, 3)])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7])
def test_windows_ref_equals_the_oracle_row_by_row(k, W, S):
    from oracle import oracle
    from phamers_amd import kmer
    from tests import windows_ref
    seqs = noisy_seqs(10 * k + S, W)
    owner, start, counts, sums = windows_ref.window_counts(seqs, k, W, S)
    plan_owner, plan_start = kmer.window_plan([len(s) for s in seqs], W, S)
    assert owner.dtype == np.int64 and start.dtype == np.int64
    assert np.array_equal(owner, plan_owner) and np.array_equal(start, plan_start)
    assert counts.dtype == np.int64 and counts.shape == (len(owner), 4 ** k)
    assert sums.dtype == np.int64 and np.array_equal(sums, counts.sum(axis=1))
    assert len(owner) >= 10 and (sums > 0).any() and (sums < W - k + 1).any()
    if S <= 6:                                      # (a larger step can miss the run of N)
        assert (sums == 0).any()
    for i, (r, a) in enumerate(zip(owner, start)):
        assert np.array_equal(counts[i], oracle.count_string(seqs[r][a:a + W], k)), (i, r, a)


def test_windows_ref_takes_no_window_and_other_symbols():
    from oracle import oracle
    from tests import windows_ref
    owner, start, counts, sums = windows_ref.window_counts(["ACG", ""], 2, 4, 1)
    assert owner.shape == start.shape == sums.shape == (0,) and counts.shape == (0, 16)
    owner, start, counts, sums = windows_ref.window_counts([], 3, 4, 1)
    assert owner.shape == (0,) and counts.shape == (0, 64)
    s = "AUGCCGUAAUGTTAUG"                            # T is no RNA symbol: invalid
    _, start, counts, _ = windows_ref.window_counts([s], 2, 6, 2, symbols="AUGC")
    for i, a in enumerate(start):
        assert np.array_equal(counts[i], oracle.count_string(s[a:a + 6], 2, symbols="AUGC"))


@pytest.mark.parametrize("k", [1, 3, 4, 5])
def test_windows_ref_folded_is_the_slice_plus_its_reverse_complement(k):
    from oracle import oracle
    from tests import strands_ref, windows_ref
    W, S = 24, 5
    seqs = noisy_seqs(k, W)
    owner, start, counts, sums = windows_ref.window_counts_folded(seqs, k, W, S)
    fwd = windows_ref.window_counts(seqs, k, W, S)
    assert np.array_equal(owner, fwd[0]) and np.array_equal(start, fwd[1])
    assert np.array_equal(sums, counts.sum(axis=1)) and np.array_equal(sums, 2 * fwd[3])
    assert np.array_equal(counts, strands_ref.fold(fwd[2]))
    for i, (r, a) in enumerate(zip(owner, start)):
        piece = seqs[r][a:a + W]
        want = oracle.count_string(piece, k) + oracle.count_string(strands_ref.revcomp(piece), k)
        assert np.array_equal(counts[i], want), (i, r, a)


def test_windows_ref_is_fast_enough_for_a_grid_pass_of_windows():
    """About 82 000 windows of 16 bases at k = 4 (the largest case of tests/test_gpu_windows_sliding.py), a sample of the
    rows against the oracle."""
    from oracle import oracle
    from tests import windows_ref
    rng = np.random.RandomState(4)
    seqs = ["".join(rng.choice(list("ATGC"), L)) for L in rng.randint(16, 19, 41000)]
    owner, start, counts, sums = windows_ref.window_counts(seqs, 4, 16, 1)
    assert 80000 < len(owner) < 84000 and (sums == 13).all()
    for i in range(0, len(owner), 4099):
        assert np.array_equal(counts[i], oracle.count_string(seqs[owner[i]][start[i]:start[i] + 16], 4))
