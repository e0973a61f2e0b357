"""CPU-only: the statements of tests/segment_fit_ref.py against the brute force over all paths, the M-step's rules, the
host half of the fit (phamers_amd/segment.py ``fit`` / ``fit_track`` / ``save_fit``, the --fit flags of
phamers_amd/windows.py) with the statements standing in for the device, and the recovery condition on the statement alone."""
import argparse
import os

import numpy as np
import pytest

from tests import segment_fit_ref as fref, segment_ref as ref


# ---- the statements ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b,s", [(0.05, 0.1, None), (0.5, 0.5, 0.5), (1e-3, 0.3, 0.9), (0.7, 0.01, None)])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 12])
def test_e_step_equals_the_brute_force_over_all_paths(n, a, b, s):
    trans, init = ref.parameters(a, b, s)
    rng = np.random.default_rng(1000 * n + int(100 * a))
    for case in range(6):
        x = ref.biased_evidence(rng, n, run=3)
        if case >= 3:                                # exact ties: evidence in whole units, some of it zero
            x = np.rint(x) * (rng.random(n) < 0.6)
        if case == 5:
            x[:] = 0.0
        xi, g0, lo = (v[0] for v in fref.expected(x, trans, init))
        bxi, bg0, blo = fref.brute_force(x, trans, init)
        assert np.allclose(xi.astype(np.float64), bxi.astype(np.float64), rtol=1e-15, atol=1e-300), (case, x)
        assert np.allclose(g0.astype(np.float64), bg0.astype(np.float64), rtol=1e-15, atol=0)
        assert abs(float(lo - blo)) <= 1e-15 * (1 + abs(float(blo)))
        assert abs(float(xi.sum()) - (n - 1)) <= 1e-15 * n and abs(float(g0.sum()) - 1) <= 1e-15
        post, _, flo = ref.forward_backward(x, trans, init)                       # and segment_ref's statement
        assert abs(float(g0[1] - post[0])) <= 1e-15 and abs(float(lo - flo)) <= 1e-15 * (1 + abs(float(flo)))
        assert np.allclose(float(xi[1] + xi[3]), float(post[1:].sum()), rtol=1e-14, atol=1e-300)
    assert not fref.expected(np.zeros(0), trans, init)[0].any()                   # no window: nothing
    one = fref.expected([1.5], trans, init)
    assert not one[0].any() and abs(float(one[1].sum()) - 1) < 1e-18                # one window: gamma_0 alone
    two = fref.expected_records([np.array([1.5]), np.zeros(0), np.array([0.5, -2.0, 1.0])], trans, init)
    assert two[0].shape == (3, 4) and not two[0][:2].any() and not two[1][1].any() and two[2][1] == 0


def test_tree_sum_is_the_rule_written_out():
    rng = np.random.default_rng(3)
    for R in (0, 1, 2, 255, 256, 257, 1000, 256 * 256 + 5):
        v = rng.random((R, 3)) * 10.0 ** rng.integers(-3, 4, (R, 1))
        got = fref.tree_sum(v)
        rows = [v[i] for i in range(R)]
        while True:                                  # the same rule in plain Python
            blocks = []
            for lo in range(0, max(len(rows), 1), 256):
                w = rows[lo:lo + 256] + [np.zeros(3)] * (256 - len(rows[lo:lo + 256]))
                s = 128
                while s:
                    w = [w[i] + w[i + s] for i in range(s)]
                    s //= 2
                blocks.append(w[0])
            rows = blocks
            if len(rows) == 1:
                break
        assert np.array_equal(got, rows[0]), R
        assert np.allclose(got, v.sum(axis=0), rtol=1e-12)
    assert [fref.tree_levels(R) for R in (1, 256, 257, 65536, 65537)] == [1, 1, 2, 2, 3]


def test_m_step_rules():
    # plain
    (a, b, s), status = fref.m_step([90.0, 10.0, 5.0, 15.0, 3.0, 1.0], (0.3, 0.3, 0.3), start_mode=fref.FIXED)
    assert (a, b, s, status) == (10.0 / (90.0 + 10.0), 5.0 / (5.0 + 15.0), 0.3, 0)
    # prior counts enter before the quotient
    (a, b, s), status = fref.m_step([90.0, 10.0, 5.0, 15.0, 3.0, 1.0], (0.3, 0.3, 0.3), (1.0, 2.0, 3.0, 4.0), fref.FIXED)
    assert (a, b) == (12.0 / (91.0 + 12.0), 8.0 / (8.0 + 19.0)) and status == 0
    # the three start modes
    assert fref.m_step([90.0, 10.0, 5.0, 15.0, 3.0, 1.0], (0.3, 0.3, 0.3), start_mode=fref.FREE)[0][2] == 1.0 / (3.0 + 1.0)
    (a, b, s), _ = fref.m_step([90.0, 10.0, 5.0, 15.0, 3.0, 1.0], (0.3, 0.3, 0.3), start_mode=fref.STATIONARY)
    assert s == a / (a + b)
    assert fref.m_step([90.0, 10.0, 5.0, 15.0, 0.0, 0.0], (0.3, 0.3, 0.3), start_mode=fref.FREE) == ((0.1, 0.25, 0.3), 0)
    # clamps
    (a, b, s), status = fref.m_step([100.0, 0.0, 7.0, 1e-20, 1.0, 0.0], (0.3, 0.3, 0.3), start_mode=fref.FREE)
    assert (a, b, s) == (1e-12, 1 - 1e-12, 1e-12) and status == fref.CLAMPED
    # a row without expected counts keeps its parameter
    (a, b, s), status = fref.m_step([0.0, 0.0, 5.0, 15.0, 1.0, 1.0], (0.3, 0.4, 0.2), start_mode=fref.FIXED)
    assert (a, b, s) == (0.3, 0.25, 0.2) and status == fref.NO_TRANSITIONS
    (a, b, s), status = fref.m_step([0.0] * 6, (0.3, 0.4, 0.2), start_mode=fref.STATIONARY)
    assert (a, b, s) == (0.3, 0.4, 0.3 / (0.3 + 0.4)) and status == fref.NO_TRANSITIONS
    # ... unless the prior gives it counts
    assert fref.m_step([0.0] * 6, (0.3, 0.4, 0.2), (3.0, 1.0, 1.0, 1.0), fref.FIXED) == ((0.25, 0.5, 0.2), 0)


def test_bounds():
    assert fref.xi_bound(4096) == ref.posterior_bound(4096) + (4096 + 16.0) * 2.0 ** -53
    d = (4096 * (4 + 2 * ref.EXP_ULP + 1 / 16.0) + 3 + 2 * ref.EXP_ULP) * fref.U      # the derivation's own terms
    assert 2 * d + 4 * fref.U + 4096 * fref.U <= fref.xi_bound(4096) < 1e-10


# ---- the recovery condition, on the statement alone ---------------------------------------------------------------------------
A_TRUE, B_TRUE = 0.004, 0.04


def recovery_case():
    """64 records of 1 500 windows from the chain (0.004, 0.04), and ``segment_track``'s default start at step 500."""
    x, states = fref.sample_chain(np.random.default_rng(7), 64, 1500, A_TRUE, B_TRUE)
    b0 = 500.0 / 30000.0
    a0 = b0 * 0.05 / (1.0 - 0.05)
    return x, states, a0, b0


def test_em_on_the_statement_recovers_the_chain():
    x, states, a0, b0 = recovery_case()
    assert 0.05 < states.mean() < 0.15
    trace, n_iter, status = fref.em(x, a0, b0, a0 / (a0 + b0), fref.FIXED, max_iter=50, tol=1e-6)
    assert status == fref.CONVERGED and 2 <= n_iter <= 50
    a, b = trace[-1][0], trace[-1][1]
    assert abs(a - A_TRUE) <= 0.2 * A_TRUE and abs(b - B_TRUE) <= 0.2 * B_TRUE, (a, b)
    L = [row[4] for row in trace]
    for before, after in zip(L[:-1], L[1:]):         # exact EM: the evidence never falls by more than rounding
        assert after - before >= -1e-9 * abs(after), L
    assert L[-1] > L[0] + 1.0
    # the stationary start, the default, meets the same condition
    trace, n_iter, status = fref.em(x, a0, b0, a0 / (a0 + b0), fref.STATIONARY, max_iter=50, tol=1e-6)
    a, b = trace[-1][0], trace[-1][1]
    assert status & fref.CONVERGED and abs(a - A_TRUE) <= 0.2 * A_TRUE and abs(b - B_TRUE) <= 0.2 * B_TRUE, (a, b)
    assert trace[-1][4] == max(row[4] for row in trace)


# ---- the host half, with the statements standing in for the device ------------------------------------------------------------
@pytest.fixture
def statement_device(monkeypatch):
    """``_lib.segment_decode`` / ``segment_fit`` replaced by the statements: the host half runs without a device."""
    from phamers_amd import _lib
    calls = []

    def pieces(x, offsets):
        return [np.asarray(x[int(offsets[r]):int(offsets[r + 1])], dtype=np.float64) for r in range(len(offsets) - 1)]

    def decode(ctx, x, offsets, trans, init, qt, qp):
        calls.append(("decode", np.array(trans), np.array(init)))
        R = len(offsets) - 1
        post, state = np.empty(len(x)), np.empty(len(x), dtype=np.uint8)
        lo, ps = np.zeros(R), np.zeros(R, dtype=np.int64)
        for r, piece in enumerate(pieces(x, offsets)):
            if len(piece):
                a, b = int(offsets[r]), int(offsets[r + 1])
                state[a:b], ps[r] = ref.viterbi(ref.quantise(piece), qt, qp)
                p, _, lo[r] = ref.forward_backward(piece, trans, init)
                post[a:b] = p.astype(np.float64)
        return post, state, lo, ps

    def fit(ctx, x, offsets, start, start_mode, prior_counts, max_iter, tol):
        calls.append(("fit", tuple(start), start_mode, tuple(prior_counts), max_iter, tol))
        trace, n_iter, status = fref.em(pieces(x, offsets), start[0], start[1], start[2], start_mode, prior_counts, max_iter, tol)
        rows = np.array([list(row[:3]) + list(row[3]) + [row[4]] for row in trace])
        return rows, n_iter, status, rows[-1, :3].copy()
    monkeypatch.setattr(_lib, "segment_decode", decode)
    monkeypatch.setattr(_lib, "segment_fit", fit)
    monkeypatch.setattr(_lib, "get_context", lambda device=None: None)
    return calls


def hand_track(scores, owner, window=500, step=500, records=("a", "b", "c")):
    from phamers_amd import windows
    owner = np.asarray(owner, dtype=np.int64)
    start = np.zeros(len(owner), dtype=np.int64)
    for r in set(owner.tolist()):
        start[owner == r] = np.arange((owner == r).sum()) * step
    return windows.WindowTrack(list(records), owner, start, window, step, np.asarray(scores, dtype=float))


def fit_track_case():
    rng = np.random.default_rng(5)
    x, _ = fref.sample_chain(rng, 2, 120, 0.05, 0.1)
    return hand_track(np.concatenate((x[0], x[1][:70])), [0] * 120 + [2] * 70)


def test_fit_track_and_segment_track_fit(statement_device):
    from phamers_amd import _lib, segment
    track = fit_track_case()
    f = segment.fit_track(track, mean_region=5000, phage_fraction=0.2, max_iter=30, tol=1e-9)
    b0 = 500 / 5000.0
    a0 = b0 * 0.2 / 0.8
    assert statement_device[-1] == ("fit", (a0, b0, a0 / (a0 + b0)), _lib.SEG_START_STATIONARY, (0.0, 0.0, 0.0, 0.0), 30, 1e-9)
    assert f.trace.shape == (f.n_iter + 1, 10) and tuple(f.trace[0, :3]) == (a0, b0, a0 / (a0 + b0))
    assert (f.p_enter, f.p_leave, f.p_start) == tuple(f.trace[-1, :3]) and f.log_evidence == f.trace[-1, 9]
    assert f.converged and not f.clamped and not f.no_transitions and f.temper == 1.0
    assert f.mean_region == 500.0 / f.p_leave and f.phage_fraction == f.p_enter / (f.p_enter + f.p_leave)
    assert f.log_evidence == f.trace[:, 9].max() > f.trace[0, 9]
    assert segment.TRACE_COLUMNS[9] == "log_evidence" and len(segment.TRACE_COLUMNS) == _lib.SEG_TRACE_COLS == 10
    # the start modes and what goes down with them
    segment.fit_track(track, p_start='free', prior_counts=(1, 2, 3, 4), max_iter=2)
    assert statement_device[-1][2:5] == (_lib.SEG_START_FREE, (1.0, 2.0, 3.0, 4.0), 2)
    segment.fit(track.scores, track.owner, 0.05, 0.1, p_start=0.25, temper=0.5, max_iter=1)
    assert statement_device[-1][1:3] == ((0.05, 0.1, 0.25), _lib.SEG_START_FIXED)
    assert segment.fit(track.scores, track.owner, 0.05, 0.1, max_iter=0).n_iter == 0
    # fit=True: the fit first, then the decode at the fitted values; the default is the decode it always was
    seg = segment.segment_track(track, mean_region=5000, phage_fraction=0.2, fit=True, max_iter=30, tol=1e-9)
    kind, trans, init = statement_device[-1]
    assert kind == "decode" and np.array_equal(trans, [1 - f.p_enter, f.p_enter, f.p_leave, 1 - f.p_leave])
    assert np.array_equal(init, [1 - f.p_start, f.p_start]) and (seg.p_enter, seg.p_leave) == (f.p_enter, f.p_leave)
    assert np.array_equal(seg.fit.trace, f.trace)
    plain = segment.segment_track(track, mean_region=5000, phage_fraction=0.2)
    assert plain.fit is None and (plain.p_enter, plain.p_leave) == (a0, b0)
    assert np.array_equal(statement_device[-1][1], [1 - a0, a0, b0, 1 - b0])
    with pytest.raises(TypeError):
        segment.segment_track(track, max_iter=3)
    with pytest.raises(TypeError):
        segment.segment_track(track, fit=True, iterations=3)


def test_argument_errors_before_any_device_work(monkeypatch):
    from phamers_amd import _lib, segment

    def no_device(*a, **kw):
        raise AssertionError("the arguments are checked before a context is asked for")
    monkeypatch.setattr(_lib, "get_context", no_device)
    x, off = np.ones(5), [0, 5]
    for kw in (dict(p_start='sideways'), dict(p_start=0.0), dict(p_start=1.0), dict(prior_counts=(0, 0, 0)),
               dict(prior_counts=(0, 0, 0, -1)), dict(prior_counts=(0, 0, 0, np.inf)), dict(max_iter=-1), dict(max_iter=2.5),
               dict(max_iter=10 ** 9), dict(tol=-1e-3), dict(tol=np.nan), dict(temper=0.0)):
        with pytest.raises(ValueError):
            segment.fit(x, off, 0.05, 0.1, **kw)
    for a, b in ((0.0, 0.1), (1.0, 0.1), (0.05, 0.0), (np.nan, 0.1), (1e-20, 0.1)):
        with pytest.raises(ValueError):
            segment.fit(x, off, a, b)
        with pytest.raises(ValueError):
            segment.expected_counts(x, off, a, b)
    with pytest.raises(ValueError):
        segment.fit([1.0, np.inf], [0, 2], 0.05, 0.1)
    with pytest.raises(ValueError):
        segment.fit(x, [0, 3, 2, 5], 0.05, 0.1)
    with pytest.raises(ValueError):
        segment.fit_track(fit_track_case(), mean_region=400)


# ---- files and the command line ------------------------------------------------------------------------------------------------
def test_fit_file_round_trip(statement_device, tmp_path):
    from phamers_amd import fileIO, segment
    f = segment.fit_track(fit_track_case(), mean_region=5000, phage_fraction=0.2, max_iter=6)
    path = str(tmp_path / "segment_fit.csv")
    args = argparse.Namespace(window=500, fit=True)
    segment.save_fit(path, f, args=args)
    text = open(path).read()
    assert text.startswith("# " + fileIO.generate_summary(args, header="PhaMers segment fit file").split("\n")[0] + "\n")
    assert "# fit:\tTrue\n" in text and ("# " + segment.FIT_COLUMNS + "\n") in text
    assert segment.FIT_COLUMNS == "iteration,p_enter,p_leave,p_start,mean_region,phage_fraction,log_evidence"
    rows = segment.read_fit(path)
    assert len(rows) == f.n_iter + 1 and [r[0] for r in rows] == list(range(f.n_iter + 1))
    for i, row in enumerate(rows):                   # repr(float) round-trips bit for bit
        assert row[1:4] == tuple(f.trace[i, :3]) and row[6] == f.trace[i, 9]
        assert row[4] == 500.0 / f.trace[i, 1] and row[5] == f.trace[i, 0] / (f.trace[i, 0] + f.trace[i, 1])
    assert rows[-1][1:6] == (f.p_enter, f.p_leave, f.p_start, f.mean_region, f.phage_fraction)
    segment.save_fit(path, f)
    assert segment.read_fit(path) == rows


def test_command_line_parses_the_fit_flags():
    from phamers_amd import windows
    a = windows._parser().parse_args(["-in", "g.fasta", "-out", "o"])
    assert (a.fit, a.fit_iterations, a.fit_tolerance, a.fit_start) == (False, 200, 1e-8, "stationary")
    a = windows._parser().parse_args("-in g.fa -out o -m likelihood -w 500 -s 500 --segment --fit --fit_iterations 50 "
                                     "--fit_tolerance 1e-6 --fit_start free".split())
    assert (a.segment, a.fit, a.fit_iterations, a.fit_tolerance, a.fit_start) == (True, True, 50, 1e-6, "free")
    with pytest.raises(SystemExit):
        windows._parser().parse_args("-in g.fa -out o --segment --fit --fit_start fixed".split())
    assert list(vars(a))[-4:] == list(windows._FIT_FLAGS)          # after every flag the parent had


PARENT_FLAGS = ("fasta_file", "output_directory", "data_directory", "positive_features", "negative_features", "window", "step",
                "kmer_length", "method", "threshold", "min_windows", "both_strands", "pseudocount", "segment", "mean_region",
                "phage_fraction", "temper")


@pytest.fixture
def fake_scoring(monkeypatch):
    """windows.main with the reference files and the device out of the way: a hand-written track."""
    from phamers_amd import phamer, windows
    track = fit_track_case()

    def load(self):
        self.positive_data, self.negative_data, self.positive_counts, self.negative_counts = "pd", "nd", "pc", "nc"
    monkeypatch.setattr(phamer.phamer_scorer, "_load_reference", load)
    monkeypatch.setattr(windows, "score_windows", lambda fasta, positive, negative, **kw: track)
    return track


def test_without_fit_the_three_files_are_what_they_were(fake_scoring, statement_device, tmp_path):
    from phamers_amd import segment, windows
    track = fake_scoring
    out = str(tmp_path / "out")
    argv = ["-in", "g.fasta", "-out", out, "-pf", "p.csv", "-nf", "n.csv", "-w", "500", "-s", "500", "-m", "likelihood", "--segment",
            "--mean_region", "5000", "--phage_fraction", "0.2"]
    windows.main(argv)
    assert sorted(os.listdir(out)) == ["phage_regions.csv", "phage_segments.csv", "window_scores.csv"]
    assert not any(call[0] == "fit" for call in statement_device)
    # the parent's Namespace: its flags, in its order -- the one it stamped phage_segments.csv with; the other two files'
    # lacks the segmentation's flags
    parsed = windows._parser().parse_args(argv)
    assert list(vars(parsed))[:len(PARENT_FLAGS)] == list(PARENT_FLAGS)
    parent = argparse.Namespace(**{name: getattr(parsed, name) for name in PARENT_FLAGS})
    shown = argparse.Namespace(**{name: getattr(parsed, name) for name in PARENT_FLAGS[:13]})
    seg = segment.segment_track(track, mean_region=5000, phage_fraction=0.2)
    assert len(seg.regions()) >= 1
    segment.save_segments(str(tmp_path / "s.csv"), seg.regions(), args=parent)
    windows.save_track(str(tmp_path / "t.csv"), track, args=shown)
    windows.save_regions(str(tmp_path / "r.csv"), windows.call_regions(track), args=shown)
    for name, mine in (("phage_segments.csv", "s.csv"), ("window_scores.csv", "t.csv"), ("phage_regions.csv", "r.csv")):
        assert open(os.path.join(out, name), "rb").read() == open(str(tmp_path / mine), "rb").read(), name
        assert "# fit" not in open(os.path.join(out, name)).read()


def test_fit_flag_decodes_with_the_fitted_chain_and_writes_the_trace(fake_scoring, statement_device, tmp_path):
    from phamers_amd import segment, windows
    track = fake_scoring
    out, plain = str(tmp_path / "out"), str(tmp_path / "plain")
    base = ["-pf", "p.csv", "-nf", "n.csv", "-w", "500", "-s", "500", "-m", "likelihood", "--segment", "--mean_region", "5000",
            "--phage_fraction", "0.2"]
    windows.main(["-in", "g.fasta", "-out", out] + base + ["--fit", "--fit_iterations", "30", "--fit_tolerance", "1e-9"])
    windows.main(["-in", "g.fasta", "-out", plain] + base)
    assert sorted(os.listdir(out)) == ["phage_regions.csv", "phage_segments.csv", "segment_fit.csv", "window_scores.csv"]
    want = segment.segment_track(track, mean_region=5000, phage_fraction=0.2, fit=True, max_iter=30, tol=1e-9)
    assert segment.read_segments(os.path.join(out, "phage_segments.csv")) == want.regions()
    rows = segment.read_fit(os.path.join(out, "segment_fit.csv"))
    assert len(rows) == want.fit.n_iter + 1 and rows[-1][1:4] == (want.p_enter, want.p_leave, want.fit.p_start)
    assert all(b[6] >= a[6] for a, b in zip(rows[:-1], rows[1:]))
    text = open(os.path.join(out, "phage_segments.csv")).read()
    assert "# fit:\tTrue\n" in text and "# fit_iterations:\t30\n" in text
    for name in ("window_scores.csv", "phage_regions.csv"):          # --fit adds nothing to the two track files
        assert open(os.path.join(out, name)).read().replace(out, plain) == open(os.path.join(plain, name)).read()
    with pytest.raises(SystemExit):
        windows.main(["-in", "g.fasta", "-out", out, "-pf", "p.csv", "-nf", "n.csv", "--fit"])
