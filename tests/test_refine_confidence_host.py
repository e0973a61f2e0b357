"""CPU-only: the host half of the boundary confidence with the statement
(tests/refine_confidence_ref.py) in the place of the device, the way tests/test_refine_host.py puts it in ``refine._refine``'s:
the statement's own edge cases; the fields of a ``Confidence`` and ``at_lo`` / ``at_hi``; the quantisation of ``drop`` and its
errors; ``ComposedSequences.refine(confidence=)`` beside the call without it; the file of ``--confidence`` and the output
directory without the flag; and the behavioural case on the statement."""
import inspect
import os

import numpy as np
import pytest

from tests import refine_confidence_ref as fref
from tests import refine_ref as rref
from tests.segment_ref import LD
from tests.test_refine_host import _fasta, _statement, _two_records
from tests.test_compose_groups_host import _old_files, _segment_on_the_host

CALLS = []


def _statement_confidence(fasta_or_sequences, kmer_length, symbols, qtable, seq, lo, x, hi, left_row, right_row, drop_q):
    """``refine._confidence`` by the statement, its sums rounded to float64; the checks the library makes are asserted."""
    seqs = rref.read_fasta(fasta_or_sequences)[1] if isinstance(fasta_or_sequences, str) else list(fasta_or_sequences)
    for b in range(len(seq)):
        assert 0 <= lo[b] <= x[b] <= hi[b] <= len(seqs[int(seq[b])])
    assert isinstance(drop_q, int) and 0 <= drop_q < 2 ** 63
    CALLS.append(drop_q)
    pos, ev, sup, interval, sums = fref.confidence(seqs, kmer_length, qtable, seq, lo, x, hi, left_row, right_row, drop_q,
                                                   symbols.decode("latin-1"))
    return pos, ev, sup, interval, sums.astype(np.float64)


@pytest.fixture
def compose(monkeypatch):
    from phamers_amd import compose as cp
    from phamers_amd import refine
    from tests import compose_groups_ref as gref
    from tests import compose_ref as cref
    monkeypatch.setattr(cp, "_estep", cref.StatementEStep)
    monkeypatch.setattr(cp, "_estep_groups", gref.StatementGroupEStep)
    monkeypatch.setattr(refine, "_refine", _statement)
    monkeypatch.setattr(refine, "_confidence", _statement_confidence)
    del CALLS[:]
    return cp


# ---- the statement itself -------------------------------------------------------------------------------------------------
def test_statement_on_cases_done_by_hand():
    # k = 1, d(A) = +1, d(T) = -1, d(G) = d(C) = 0 in units of one nat (2^16)
    one = 1 << 16
    q = np.array([[one, -one, 0, 0], [0, 0, 0, 0]], dtype=np.int64)
    #      P:  0 1 0 0 0 1 0     two maxima (p = 1 and p = 5, a tie class split in two), the dip between them one nat deep
    seq = "ATGGAT"
    st = fref.Statement([seq], 1, q, [0], [0], [3], [6], [0], [1])
    assert st.P[0] == [0, one, 0, 0, 0, one, 0] and st.position[0] == 1 and st.n[0] == 7
    assert st.interval(0).tolist() == [[1, 5, 2]]                           # not contiguous: n_within < upper - lower + 1
    assert st.interval(one - 1).tolist() == [[1, 5, 2]] and st.interval(one).tolist() == [[0, 6, 7]]
    Z, M, left, right, S2 = st.sums(0)[0]
    e = np.exp(LD(-1))
    assert abs(Z - (2 + 5 * e)) < 1e-17 and abs(M - (2 + 3 * e)) < 1e-17   # M counts the dip
    assert left == e and abs(right - (e * (1 + 2 + 3 + 5) + 4)) < 1e-17
    assert abs(S2 - (e * (1 + 1 + 4 + 9 + 25) + 16)) < 1e-16
    # the cut: 701 nats below the maximum weighs 0 exactly, 700 nats does not
    big = np.array([[700 * one, -701 * one, 0, 0], [0, 0, 0, 0]], dtype=np.int64)
    st = fref.Statement(["AT", "TA"], 1, big, [0, 1], [0, 0], [0, 0], [2, 2], [0, 0], [1, 1])
    assert st.P == [[0, 700 * one, -one], [0, -701 * one, -one]] and st.position.tolist() == [1, 0]
    s = st.sums(0)
    assert s[0, 2] == np.exp(LD(-700)) > 0 and s[0, 3] == 0                 # p = 0 at 700 nats weighs, p = 2 at 701 does not
    assert s[1, 0] == 1 + np.exp(LD(-1)) and s[1, 2] == 0 and s[1, 3] == 2 * np.exp(LD(-1))
    # an empty interval
    st = fref.Statement(["ACGT"], 1, q, [0], [2], [2], [2], [0], [1])
    assert st.interval(5).tolist() == [[2, 2, 1]] and st.sums(5).tolist() == [[1, 1, 0, 0, 0]]
    assert fref.sum_bound(1) < fref.sum_bound(2049) < 2049 * 1.01 * 2.0 ** -53 + 8 * 2.0 ** -53


# ---- refine.confidence ------------------------------------------------------------------------------------------------------
def test_confidence_fields_and_drop(compose):
    from phamers_amd import refine, segment
    rng = np.random.default_rng(5)
    seqs = ["".join("ATGC"[d] for d in rng.integers(0, 4, 300)), "ACGTNACGTTTGACCA"]
    logp = np.log(rng.dirichlet(np.ones(16), 3))
    args = dict(seq=[0, 1, 0, 0], lo=[10, 0, 50, 0], x=[100, 8, 50, 150], hi=[250, 16, 50, 300], left_row=[0, 1, 2, 2],
                right_row=[1, 2, 0, 1])
    assert list(inspect.signature(refine.confidence).parameters) == [
        "fasta_or_sequences", "kmer_length", "log_profiles", "seq", "lo", "x", "hi", "left_row", "right_row", "drop", "symbols"]
    assert inspect.signature(refine.confidence).parameters["drop"].default == 3.0
    assert "modelling choice" in refine.confidence.__doc__
    plain = refine.boundaries(seqs, 2, logp, **args)
    for drop, drop_q in ((3.0, 3 << 16), (0, 0), (0.5, 1 << 15), (2.0 ** -17, 1), (2.0 ** -18, 0), (1e-5, 1), (1e300, 1 << 62)):
        r, c = refine.confidence(seqs, 2, logp, drop=drop, **args)
        assert CALLS[-1] == drop_q == (1 << 62 if drop == 1e300 else int(np.floor(drop * 65536 + 0.5)))
        for name, g, w in zip(r._fields, r, plain):
            assert np.array_equal(g, w), name
        pos, ev, sup, interval, sums = fref.confidence(seqs, 2, segment.quantise(logp), drop_q=drop_q, **args)
        assert c._fields == ("lower", "upper", "n_within", "at_lo", "at_hi", "log_z", "mass_at_position", "mass_within",
                             "mean_offset", "rms_distance", "sums")
        assert np.array_equal(np.stack([c.lower, c.upper, c.n_within], axis=1), interval)
        assert c.lower.dtype == c.upper.dtype == c.n_within.dtype == np.int64 and c.at_lo.dtype == c.at_hi.dtype == bool
        assert np.array_equal(c.at_lo, interval[:, 0] == args["lo"]) and np.array_equal(c.at_hi, interval[:, 1] == args["hi"])
        assert np.array_equal(c.sums, sums.astype(np.float64)) and c.sums.dtype == np.float64
        Z, M, left, right, S2 = (c.sums[:, i] for i in range(5))
        assert np.array_equal(c.log_z, np.log(Z)) and np.array_equal(c.mass_at_position, 1.0 / Z)
        assert np.array_equal(c.mass_within, M / Z) and np.array_equal(c.mean_offset, (right - left) / Z)
        assert np.array_equal(c.rms_distance, np.sqrt(S2 / Z))
        fref.assert_derived_within(c, sums, [h - l + 1 for l, h in zip(args["lo"], args["hi"])])
        assert (c.lower <= r.position).all() and (r.position <= c.upper).all() and (c.n_within >= 1).all()
        assert (c.n_within <= c.upper - c.lower + 1).all() and (Z >= 1).all() and (c.mass_within <= 1 + 1e-12).all()
        assert c.lower[2] == c.upper[2] == 50 and c.n_within[2] == 1 and c.at_lo[2] and c.at_hi[2]      # the empty interval
        assert c.sums[2].tolist() == [1, 1, 0, 0, 0] and c.mass_within[2] == 1 and c.rms_distance[2] == 0
    r, c = refine.confidence(seqs, 2, logp, drop=1e300, **args)             # every candidate
    assert c.at_lo.all() and c.at_hi.all() and np.array_equal(c.n_within, np.array(args["hi"]) - args["lo"] + 1)
    assert np.array_equal(c.sums[:, 0], c.sums[:, 1])
    r, c = refine.confidence(seqs, 2, logp, **args)                           # the default is 3 nats
    assert CALLS[-1] == 3 << 16
    none = refine.confidence(seqs, 2, logp, [], [], [], [], [], [])
    assert len(none[0].position) == 0 and none[1].lower.shape == (0,) and none[1].sums.shape == (0, 5)
    for bad in (-1, -1e-9, float("nan"), float("inf"), -float("inf"), "much", None):
        with pytest.raises(ValueError):
            refine.confidence(seqs, 2, logp, drop=bad, **args)
    with pytest.raises(ValueError):
        refine.confidence(seqs, 2, logp, drop=1.0, **dict(args, lo=[101, 0, 50, 0]))                      # boundaries' own checks
    assert refine.drop_quantum(3) == 196608 and refine.drop_quantum(np.float32(0.25)) == 16384


# ---- ComposedSequences.refine(confidence=) and the command line -------------------------------------------------------------
def _same_boundaries(a, b):
    for name, g, w in zip(a._fields, a, b):
        assert (g == w) if isinstance(g, list) else np.array_equal(g, w), name


def test_composed_sequences_refine_with_confidence(compose, tmp_path):
    seqs = _two_records()
    path = _fasta(tmp_path, seqs)
    host = _segment_on_the_host(compose)
    plain = host(path, 3, max_iter=3).refine(seqs)
    assert plain.boundary_confidence is None and CALLS == []
    assert list(inspect.signature(compose.ComposedSequences.refine).parameters) == ["self", "fasta_or_sequences", "span", "confidence"]
    for confidence, drop_q in ((True, 3 << 16), (1.5, 3 << 15), (0, 0), (np.float64(2), 2 << 16)):
        result = host(path, 3, max_iter=3).refine(seqs, None, confidence)
        assert CALLS[-1] == drop_q
        _same_boundaries(result.boundaries, plain.boundaries)
        assert result.refined_regions() == plain.refined_regions() and result.regions() == plain.regions()
        c, b = result.boundary_confidence, result.boundaries
        assert len(c.lower) == len(b.position) >= 2
        assert (c.lower <= b.position).all() and (b.position <= c.upper).all()
        # against the statement on the plan of the decode
        rec, x, lo, hi, ls, rs, _ = rref.boundary_plan(result.state, result.owner, result.start, 500, 500)
        from phamers_amd import segment
        want = fref.confidence(seqs, 4, segment.quantise(result.composition.log_profiles), rec, lo, x, hi, ls, rs, drop_q)
        assert np.array_equal(np.stack([c.lower, c.upper, c.n_within], axis=1), want[3])
        assert np.array_equal(c.at_lo, want[3][:, 0] == lo) and np.array_equal(c.at_hi, want[3][:, 1] == hi)
        assert np.array_equal(c.sums, want[4].astype(np.float64))
    n = len(CALLS)
    for off in (None, False):
        result = host(path, 3, max_iter=3).refine(seqs, None, off)
        assert result.boundary_confidence is None and len(CALLS) == n
        _same_boundaries(result.boundaries, plain.boundaries)
    again = result.refine(seqs, confidence=True).refine(seqs)               # the call without it clears what an earlier one left
    assert again.boundary_confidence is None
    narrow = host(path, 3, max_iter=3).refine(path, 40, True)               # a span, and the file instead of the strings
    assert ((narrow.boundary_confidence.upper - narrow.boundary_confidence.lower) <= 80).all()
    per = host(path, 2, per_record=True, max_iter=3).refine(seqs, confidence=True)
    assert len(per.boundary_confidence.lower) == len(per.boundaries.position) >= 1
    for bad in (-1, float("nan"), "yes", [3]):
        with pytest.raises(ValueError):
            host(path, 3, max_iter=3).refine(seqs, None, bad)
    with pytest.raises(ValueError):
        compose.write_confidence_file(str(tmp_path / "none"), plain)


def test_segment_sequences_takes_confidence():
    """The public signature; ``confidence`` needs ``refine`` and is checked before any device work."""
    from phamers_amd import compose
    assert inspect.signature(compose.segment_sequences).parameters["confidence"].default is None
    with pytest.raises(ValueError, match="refine"):
        compose.segment_sequences(["ACGT" * 500], 2, confidence=True)
    with pytest.raises(ValueError, match="refine"):
        compose.segment_sequences(["ACGT" * 500], 2, confidence=2.0)
    with pytest.raises(ValueError):
        compose.segment_sequences(["ACGT" * 500], 2, refine=True, confidence=-2.0)


def test_command_line_files(compose, tmp_path, monkeypatch):
    monkeypatch.setattr(compose, "segment_sequences", _segment_on_the_host(compose))
    seqs = _two_records()
    fasta = _fasta(tmp_path, seqs)
    four = ["compose_profiles.csv", "compose_segments.csv", "compose_trace.csv", "compose_windows.csv"]
    six = sorted(four + ["compose_boundaries.csv", "compose_segments_refined.csv"])
    # without the flag: today's files with today's bytes
    old_dir, ref_dir = str(tmp_path / "old"), str(tmp_path / "refined")
    result = compose.main(["-in", fasta, "-out", old_dir, "-S", "3", "--max_iter", "3"])
    assert sorted(os.listdir(old_dir)) == four and result.boundaries is None and result.boundary_confidence is None
    for name, text in _old_files(old_dir, result).items():
        assert open(os.path.join(old_dir, name)).read() == text, name
    refined = compose.main(["-in", fasta, "-out", ref_dir, "-S", "3", "--max_iter", "3", "--refine"])
    assert sorted(os.listdir(ref_dir)) == six and refined.boundary_confidence is None and CALLS == []
    b = refined.boundaries
    assert open(os.path.join(ref_dir, "compose_boundaries.csv")).read() == (
        "record_id,window_boundary,position,left_state,right_state,gain,left_evidence,right_evidence,support\n" + "".join(
            "%s,%d,%d,%d,%d,%r,%r,%r,%d\n" % (b.record_id[i], b.window_boundary[i], b.position[i], b.left_state[i], b.right_state[i],
                                             float(b.gain[i]), float(b.left_evidence[i]), float(b.right_evidence[i]), b.support[i])
            for i in range(len(b.position))))
    assert open(os.path.join(ref_dir, "compose_segments_refined.csv")).read() == (
        "record_id,start,end,state,n_windows,mean_posterior\n" + "".join("%s,%d,%d,%d,%d,%r\n" % r for r in refined.refined_regions()))
    # with it: the same six files, byte for byte, and one more
    for extra, drop_q, name in ((["--confidence"], 3 << 16, "c3"), (["--confidence", "0.5"], 1 << 15, "c05"),
                                (["--refine", "60", "--confidence", "0"], 0, "c0")):
        new_dir = str(tmp_path / name)
        argv = ["-in", fasta, "-out", new_dir, "-S", "3", "--max_iter", "3"] + (extra if "--refine" in extra else ["--refine"] + extra)
        got = compose.main(argv)
        assert CALLS[-1] == drop_q
        assert sorted(os.listdir(new_dir)) == sorted(six + ["compose_boundary_confidence.csv"])
        if "60" not in extra:
            for f in six:
                assert open(os.path.join(new_dir, f)).read() == open(os.path.join(ref_dir, f)).read(), f
        b, c = got.boundaries, got.boundary_confidence
        lines = open(os.path.join(new_dir, "compose_boundary_confidence.csv")).read().splitlines()
        assert lines[0] == ("record_id,window_boundary,position,lower,upper,n_within,at_lo,at_hi,mass_within,mass_at_position,"
                            "mean_offset,rms_distance")
        assert len(lines) == 1 + len(b.position) and len(b.position) >= 2
        for i, line in enumerate(lines[1:]):
            assert line == "%s,%d,%d,%d,%d,%d,%d,%d,%r,%r,%r,%r" % (
                b.record_id[i], b.window_boundary[i], b.position[i], c.lower[i], c.upper[i], c.n_within[i], c.at_lo[i], c.at_hi[i],
                float(c.mass_within[i]), float(c.mass_at_position[i]), float(c.mean_offset[i]), float(c.rms_distance[i]))
            cells = line.split(",")
            assert len(cells) == 12 and cells[6] in "01" and cells[7] in "01" and int(cells[3]) <= int(cells[2]) <= int(cells[4])
    # the errors: --confidence without --refine, a negative or non-finite drop
    for argv in (["--confidence"], ["--confidence", "2"], ["--refine", "--confidence", "-1"], ["--refine", "--confidence", "nan"]):
        with pytest.raises(SystemExit):
            compose.main(["-in", fasta, "-out", str(tmp_path / "bad"), "-S", "3"] + argv)
    assert not os.path.exists(str(tmp_path / "bad"))
    # --per_record
    per = compose.main(["-in", fasta, "-out", str(tmp_path / "per"), "-S", "2", "--max_iter", "3", "--per_record", "--refine", "--confidence"])
    assert "compose_boundary_confidence.csv" in os.listdir(str(tmp_path / "per")) and len(per.boundary_confidence.lower) >= 1


# ---- the behavioural case on the statement --------------------------------------------------------------------------------
def test_the_join_lies_in_the_interval_and_a_close_pair_is_wider(compose):
    from phamers_amd import refine
    widths = {}
    for kind in ("far", "close"):
        cases = [fref.behaviour_case(kind, seed) for seed in fref.BEHAVIOUR_SEEDS]
        widths[kind] = []
        for seq, logp in cases:
            r, c = refine.confidence([seq], 4, logp, [0], [fref.BEHAVIOUR_LO], [fref.BEHAVIOUR_X], [fref.BEHAVIOUR_HI], [0], [1], drop=3.0)
            assert c.lower[0] <= fref.BEHAVIOUR_JOIN <= c.upper[0], (kind, c.lower, c.upper)
            assert not c.at_lo[0] and not c.at_hi[0]
            widths[kind].append(int(c.upper[0] - c.lower[0]))
    assert widths == fref.BEHAVIOUR_STATEMENT_WIDTHS
    assert np.median(widths["close"]) > np.median(widths["far"])
