"""CPU-only: the host half of the track segmentation (phamers_amd/segment.py, the new flags of phamers_amd/windows.py) and
the statements of tests/segment_ref.py against the brute force over all paths."""
import argparse
import os

import numpy as np
import pytest

from tests import segment_ref as ref


# ---- the statements ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b,s", [(0.05, 0.1, None), (0.5, 0.5, 0.5), (1e-3, 0.3, 0.9), (0.7, 0.01, None)])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 12])
def test_statements_equal_the_brute_force_over_all_paths(n, a, b, s):
    from phamers_amd import segment
    trans, init, qt, qp = segment.parameters(a, b, s)
    rng = np.random.default_rng(1000 * n + int(100 * a))
    for case in range(6):
        x = ref.biased_evidence(rng, n, run=3)
        if case >= 3:                                # exact ties: evidence in whole units, some of it zero
            x = np.rint(x) * (rng.random(n) < 0.6)
        if case == 5:
            x[:] = 0.0
        path, score, marginal, log_odds = ref.brute_force(x, trans, init, qt, qp)
        states, got_score = ref.viterbi(ref.quantise(x), qt, qp)
        assert np.array_equal(states, path) and got_score == score, (case, x)
        post, one_minus, lo = ref.forward_backward(x, trans, init)
        assert np.allclose(post.astype(np.float64), marginal.astype(np.float64), rtol=1e-15, atol=0)
        assert np.allclose((post + one_minus).astype(np.float64), 1.0, rtol=1e-15)
        assert abs(float(lo - log_odds)) <= 1e-15 * (1 + abs(float(log_odds)))


def test_all_ties_give_the_all_host_path():
    from phamers_amd import segment
    trans, init, qt, qp = segment.parameters(0.5, 0.5)
    assert len(set(qt.tolist()) | set(qp.tolist())) == 1
    states, score = ref.viterbi([0] * 9, qt, qp)
    assert not states.any() and score == 9 * int(qt[0])
    path, best, _, _ = ref.brute_force(np.zeros(9), trans, init, qt, qp)
    assert not path.any() and best == score
    assert ref.viterbi([], qt, qp)[1] == 0


def test_bounds_grow_linearly_and_hold_the_measured_constant():
    assert ref.EXP_ULP == 2.0 * ref.EXP_ULP_MEASURED
    assert ref.posterior_bound(4096) == 2.0 * (4096 * (5.0 + 2.0 * ref.EXP_ULP) + 16.0) * 2.0 ** -53
    assert ref.posterior_bound(2 ** 20) < 1e-8 and ref.log_odds_bound(np.zeros(10), 0.0) < 1e-13


# ---- parameters, quantiser, evidence ------------------------------------------------------------------------------------------
def test_parameter_rules():
    from phamers_amd import segment
    trans, init, qt, qp = segment.parameters(0.05, 0.1)
    assert np.array_equal(trans, [0.95, 0.05, 0.1, 0.9]) and np.array_equal(init, [1 - 0.05 / (0.05 + 0.1), 0.05 / (0.05 + 0.1)])
    assert qt.dtype == qp.dtype == np.int64
    assert np.array_equal(qt, np.rint(np.log(trans) * 65536)) and np.array_equal(qp, np.rint(np.log(init) * 65536))
    assert np.array_equal(segment.parameters(0.05, 0.1, 0.25)[1], [0.75, 0.25])
    t, i = ref.parameters(0.05, 0.1)
    assert np.array_equal(t, trans) and np.array_equal(i, init)
    for a, b, s in ((0.0, 0.1, None), (1.0, 0.1, None), (0.1, 0.0, None), (0.1, 1.0, None), (-0.1, 0.1, None), (np.nan, 0.1, None),
                    (0.1, np.inf, None), (0.1, 0.1, 0.0), (0.1, 0.1, 1.0), (1e-17, 0.1, None), (0.0, 0.0, None)):
        with pytest.raises(ValueError):
            segment.parameters(a, b, s)
    for a in (1e-12, 1 - 1e-12):                     # the rows sum to 1 exactly
        trans = segment.parameters(a, a)[0]
        assert trans[0] + trans[1] == 1.0 and trans[2] + trans[3] == 1.0


def test_quantiser():
    from phamers_amd import segment
    h = 2.0 ** -17                                   # half a unit
    q = segment.quantise([0.0, -0.0, h, -h, 3 * h, -3 * h, 5 * h, 1.0, -1.0, 2.0 ** 15, 2.0 ** 15 + 1, 1e300, -1e300,
                          -2.0 ** 15 - 0.5, 1e-9])
    assert q.dtype == np.int64
    assert q.tolist() == [0, 0, 0, 0, 2, -2, 2, 65536, -65536, 2 ** 31, 2 ** 31, 2 ** 31, -2 ** 31, -2 ** 31, 0]
    assert segment.quantise(-0.0).tolist() == 0 and not np.signbit(segment.quantise(-0.0))
    rng = np.random.default_rng(3)
    v = np.concatenate((rng.standard_normal(1000) * 50, rng.standard_normal(100) * 1e5))
    assert segment.quantise(v).tolist() == ref.quantise(v)
    assert segment.CLAMP == ref.CLAMP == 2.0 ** 15 and segment.QUANT_BITS == ref.QUANT_BITS == 16


def test_evidence_and_offsets():
    from phamers_amd import segment
    x = segment.evidence([1.5, np.nan, -2.0], 0.5)
    assert x.dtype == np.float64 and x.tolist() == [0.75, 0.0, -1.0]
    for bad in (dict(scores=[1.0, np.inf]), dict(scores=[1.0], temper=0.0), dict(scores=[1.0], temper=-1.0),
                dict(scores=[1.0], temper=np.nan), dict(scores=[1e308], temper=10.0), dict(scores=[[1.0]])):
        with pytest.raises(ValueError):
            segment.evidence(**bad)
    assert segment._offsets(np.array([0, 0, 2, 2, 2]), 5).tolist() == [0, 2, 2, 5]        # owners: record 1 has no window
    assert segment._offsets([0, 2, 2, 5], 5).tolist() == [0, 2, 2, 5]
    assert segment._offsets([0, 0, 0], 0).tolist() == [0, 0, 0] and segment._offsets(np.zeros(0, dtype=np.int64), 0).tolist() == [0]
    assert segment._offsets(np.zeros(2, dtype=np.int64), 2).tolist() == [0, 2]               # (n,) entries are owners
    for bad, n in (([1, 5], 5), ([0, 4], 5), ([0, 3, 2, 5], 5), ([0, 1, 0, 1, 1], 5), ([0.0, 5.0], 5), ([[0, 5]], 5), ([-1, 5], 5)):
        with pytest.raises(ValueError):
            segment._offsets(np.array(bad), n)


def test_default_temper():
    from phamers_amd import segment
    assert segment.default_temper(500, 500, 4) == 1.0 and segment.default_temper(500, 497, 4) == 1.0
    assert segment.default_temper(5000, 500, 4) == 500.0 / 4997.0
    assert segment.default_temper(1000, 200, 6) == 200.0 / 995.0
    assert segment.default_temper(4, 1, 4) == 1.0


# ---- Segmentation, its regions and file, with the statements standing in for the device --------------------------------------
@pytest.fixture
def statement_decode(monkeypatch):
    """``_lib.segment_decode`` replaced by statements (i) and (ii): the host half runs without a device."""
    from phamers_amd import _lib
    calls = []

    def decode(ctx, x, offsets, trans, init, qt, qp):
        calls.append((np.array(x), np.array(offsets), np.array(trans), np.array(init)))
        R = len(offsets) - 1
        post, state = np.empty(len(x)), np.empty(len(x), dtype=np.uint8)
        lo, ps = np.zeros(R), np.zeros(R, dtype=np.int64)
        for r in range(R):
            a, b = int(offsets[r]), int(offsets[r + 1])
            if b > a:
                state[a:b], ps[r] = ref.viterbi(ref.quantise(x[a:b]), qt, qp)
                p, _, lo[r] = ref.forward_backward(x[a:b], trans, init)
                post[a:b] = p.astype(np.float64)
        return post, state, lo, ps
    monkeypatch.setattr(_lib, "segment_decode", decode)
    monkeypatch.setattr(_lib, "get_context", lambda device=None: None)
    return calls


def hand_track(scores, owner, window=500, step=500, records=("a", "b", "c")):
    from phamers_amd import windows
    owner = np.asarray(owner, dtype=np.int64)
    start = np.zeros(len(owner), dtype=np.int64)
    for r in set(owner.tolist()):
        start[owner == r] = np.arange((owner == r).sum()) * step
    return windows.WindowTrack(list(records), owner, start, window, step, np.asarray(scores, dtype=float))


def test_segment_track_parameters_regions_and_file(statement_decode, tmp_path):
    from phamers_amd import fileIO, segment
    nan = float("nan")
    scores = [-5.0, 9.0, nan, 8.0, -6.0, -7.0] + [7.0, 7.0] + [-4.0]
    track = hand_track(scores, [0] * 6 + [2] * 2 + [2])
    track.start[8] = 1000
    seg = segment.segment_track(track, mean_region=2000, phage_fraction=0.2)
    x, off, trans, init = statement_decode[-1]
    b, a = 500 / 2000.0, (500 / 2000.0) * 0.2 / 0.8
    assert (seg.p_leave, seg.p_enter, seg.temper) == (b, a, 1.0)
    assert np.array_equal(trans, [1 - a, a, b, 1 - b]) and np.array_equal(init, [1 - a / (a + b), a / (a + b)])
    assert off.tolist() == [0, 6, 6, 9] and x.tolist() == [-5.0, 9.0, 0.0, 8.0, -6.0, -7.0, 7.0, 7.0, -4.0]
    assert seg.state.tolist() == [0, 1, 1, 1, 0, 0, 1, 1, 0]           # the chain carries across the nan window
    assert len(seg) == 9 and seg.log_odds.shape == (3,) and seg.log_odds[1] == 0.0 and seg.path_score[1] == 0.0
    regions = seg.regions()
    assert [r[:4] for r in regions] == [("a", 500, 2000, 3), ("c", 0, 1000, 2)]
    assert regions[0][4] == float(seg.posterior[1:4].mean()) and regions[0][5] == float(seg.posterior[1:4].max())
    assert regions[0][6] == 17.0 and regions[1][6] == 14.0
    assert [r[:4] for r in seg.regions(min_windows=3)] == [("a", 500, 2000, 3)]
    assert seg.regions(min_windows=4) == []
    path = str(tmp_path / "phage_segments.csv")
    args = argparse.Namespace(window=500, segment=True)
    segment.save_segments(path, regions, args=args)
    text = open(path).read()
    assert text.startswith("# " + fileIO.generate_summary(args, header="PhaMers phage segment file").split("\n")[0] + "\n")
    assert "# segment:\tTrue\n" in text and ("# " + segment.COLUMNS + "\n") in text
    assert segment.read_segments(path) == regions                       # repr(float) round-trips bit for bit
    segment.save_segments(path, [("rec,with comma", 0, 500, 1, 0.1 + 0.2, 1.0, -3.5e-7)])
    assert segment.read_segments(path) == [("rec,with comma", 0, 500, 1, 0.1 + 0.2, 1.0, -3.5e-7)]
    # overlapping windows are tempered by default; a temper of the caller's is taken as it is
    over = hand_track(scores, [0] * 9, window=5000, step=500)
    assert segment.segment_track(over).temper == 500.0 / 4997.0
    assert np.array_equal(statement_decode[-1][0][:2], np.array([-5.0, 9.0]) * (500.0 / 4997.0))
    assert segment.segment_track(over, temper=0.5, kmer_length=6).temper == 0.5
    assert segment.segment_track(over, kmer_length=6).temper == 500.0 / 4995.0
    # no window at all
    none = segment.segment_track(hand_track([], []))
    assert len(none) == 0 and none.regions() == [] and none.log_odds.tolist() == [0.0, 0.0, 0.0]
    for kw in (dict(mean_region=500), dict(mean_region=499), dict(mean_region=0), dict(phage_fraction=0.0),
               dict(phage_fraction=1.0), dict(temper=0.0)):
        with pytest.raises(ValueError):
            segment.segment_track(track, **kw)


def test_decode_takes_owners_or_offsets(statement_decode):
    from phamers_amd import segment
    scores = np.array([1.0, 2.0, -3.0, 4.0])
    d = segment.decode(scores, [0, 0, 0, 3], 0.05, 0.1)
    e = segment.decode(scores, [0, 3, 3, 3, 4], 0.05, 0.1)
    assert statement_decode[0][1].tolist() == statement_decode[1][1].tolist() == [0, 3, 3, 3, 4]
    with pytest.raises(ValueError, match="both as owners and as offsets"):
        segment.decode(scores, [0, 2, 2, 4], 0.05, 0.1)
    assert all(np.array_equal(u, v) for u, v in zip(d, e))
    assert d.path_score_q.dtype == np.int64 and np.array_equal(d.path_score, d.path_score_q * 2.0 ** -16)
    assert d._fields == ("posterior", "state", "log_odds", "path_score", "path_score_q")


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_command_line_parses_the_new_flags():
    from phamers_amd import windows
    a = windows._parser().parse_args(["-in", "g.fasta", "-out", "o"])
    assert (a.pseudocount, a.segment, a.mean_region, a.phage_fraction, a.temper) == (0.5, False, 30000, 0.05, None)
    a = windows._parser().parse_args("-in g.fa -out o -m likelihood -w 500 -s 500 --pseudocount 0.25 --segment --mean_region 20000 "
                                     "--phage_fraction 0.1 --temper 0.5".split())
    assert (a.method, a.window, a.step, a.pseudocount, a.segment, a.mean_region, a.phage_fraction, a.temper) == \
        ("likelihood", 500, 500, 0.25, True, 20000.0, 0.1, 0.5)
    assert "-m likelihood -w 500 -s 500 --segment" in " ".join(windows._parser().format_help().split())


PARENT_FLAGS = ("fasta_file", "output_directory", "data_directory", "positive_features", "negative_features", "window", "step",
                "kmer_length", "method", "threshold", "min_windows", "both_strands")


@pytest.fixture
def fake_scoring(monkeypatch):
    """windows.main with the reference files and the device out of the way: a hand-written track."""
    from phamers_amd import phamer, windows
    seen = {}
    track = hand_track([0.1 + 0.2, float("nan"), 5.0, 6.0, -3.5e-7, 2.0], [0, 0, 0, 0, 1, 1], records=("rec,with comma", "b"))

    def load(self):
        seen["keep_counts"] = self.keep_reference_counts
        self.positive_data, self.negative_data, self.positive_counts, self.negative_counts = "pd", "nd", "pc", "nc"

    def score_windows(fasta, positive, negative, **kw):
        seen.update(kw, positive=positive, negative=negative)
        return track
    monkeypatch.setattr(phamer.phamer_scorer, "_load_reference", load)
    monkeypatch.setattr(windows, "score_windows", score_windows)
    return track, seen


def test_without_the_new_flags_the_two_files_are_what_they_were(fake_scoring, tmp_path):
    from phamers_amd import windows
    track, seen = fake_scoring
    out = str(tmp_path / "out")
    argv = ["-in", "g.fasta", "-out", out, "-pf", "p.csv", "-nf", "n.csv", "-w", "500", "-s", "500", "-t", "0.2", "-min", "2"]
    got_track, regions = windows.main(argv)
    assert got_track is track and seen["method"] == "combo" and (seen["positive"], seen["negative"]) == ("pd", "nd")
    assert seen["keep_counts"] is False
    assert sorted(os.listdir(out)) == ["phage_regions.csv", "window_scores.csv"]
    # the parent's argument summary: its flags, in its order
    parsed = windows._parser().parse_args(argv)
    parent = argparse.Namespace(**{name: getattr(parsed, name) for name in PARENT_FLAGS})
    assert list(vars(parsed))[:len(PARENT_FLAGS)] == list(PARENT_FLAGS)
    windows.save_track(str(tmp_path / "t.csv"), track, args=parent)
    windows.save_regions(str(tmp_path / "r.csv"), windows.call_regions(track, threshold=0.2, min_windows=2), args=parent)
    assert open(os.path.join(out, "window_scores.csv"), "rb").read() == open(str(tmp_path / "t.csv"), "rb").read()
    assert open(os.path.join(out, "phage_regions.csv"), "rb").read() == open(str(tmp_path / "r.csv"), "rb").read()
    text = open(os.path.join(out, "window_scores.csv")).read()
    assert "# segment:" not in text and "# pseudocount:" not in text and "# temper:" not in text


def test_segment_flag_adds_one_file_and_likelihood_loads_counts(fake_scoring, statement_decode, tmp_path):
    from phamers_amd import segment, windows
    track, seen = fake_scoring
    out = str(tmp_path / "out")
    windows.main(["-in", "g.fasta", "-out", out, "-pf", "p.csv", "-nf", "n.csv", "-w", "500", "-s", "500", "-m", "likelihood",
                  "--pseudocount", "0.25", "--segment", "--mean_region", "2000", "--phage_fraction", "0.2"])
    assert seen["keep_counts"] is True and (seen["positive"], seen["negative"]) == ("pc", "nc") and seen["pseudocount"] == 0.25
    assert sorted(os.listdir(out)) == ["phage_regions.csv", "phage_segments.csv", "window_scores.csv"]
    want = segment.segment_track(track, mean_region=2000, phage_fraction=0.2).regions()
    assert segment.read_segments(os.path.join(out, "phage_segments.csv")) == want and len(want) >= 1
    # --segment adds nothing to the two existing files: they are byte for byte those of the run without the flag, whose
    # argument summary names the pseudocount because the likelihood method uses it
    plain = str(tmp_path / "plain")
    windows.main(["-in", "g.fasta", "-out", plain, "-pf", "p.csv", "-nf", "n.csv", "-w", "500", "-s", "500", "-m", "likelihood",
                  "--pseudocount", "0.25"])
    assert sorted(os.listdir(plain)) == ["phage_regions.csv", "window_scores.csv"]
    for name in ("window_scores.csv", "phage_regions.csv"):
        text = open(os.path.join(out, name)).read().replace(out, plain)
        assert text == open(os.path.join(plain, name)).read()
        assert "# pseudocount:\t0.25\n" in text and "# segment:" not in text and "mean_region" not in text


def test_likelihood_windows_refuse_frequencies_before_any_device_work(monkeypatch):
    from phamers_amd import _lib, windows

    def no_device(*a, **kw):
        raise AssertionError("the arguments are checked before a context is asked for")
    monkeypatch.setattr(_lib, "get_context", no_device)
    counts = np.arange(512).reshape(2, 256)
    with pytest.raises(ValueError, match="not frequencies"):
        windows.score_windows(["ACGT" * 200], counts / counts.sum(axis=1, keepdims=True), counts, window=500, step=500,
                              method='likelihood')
    with pytest.raises(ValueError):
        windows.score_windows(["ACGT" * 200], counts, counts, window=500, step=500, method='likelihood', pseudocount=0.0)
    with pytest.raises(ValueError):
        windows.score_windows(["ACGT" * 200], counts[:, :64], counts[:, :64], window=500, step=500, method='likelihood')
    track = windows.WindowTrack(["a"], [0], [0], 500, 500, [1.0])
    assert track.l_pos is None and track.l_neg is None
