"""CPU-only: the host half of the boundary refinement.  ``compose.boundary_plan`` equals its loop
(tests/refine_ref.py) on runs of 1, 2 and many windows, several records, window = / > / < step and spans smaller and larger
than a run, and its intervals are disjoint and ordered; ``refined_regions``, ``segment_sequences(refine=)`` and the files of
``--refine`` with the statement in the place of the device; without the flag the output directory is what it was; the
argument errors."""
import os

import numpy as np
import pytest

from tests import compose_ref as cref
from tests import refine_ref as rref
from tests.test_compose_groups_host import _old_files, _segment_on_the_host


def _statement(fasta_or_sequences, kmer_length, symbols, qtable, seq, lo, x, hi, left_row, right_row):
    """``refine._refine`` by the statement; the checks the library makes are asserted."""
    seqs = rref.read_fasta(fasta_or_sequences)[1] if isinstance(fasta_or_sequences, str) else list(fasta_or_sequences)
    for b in range(len(seq)):
        assert 0 <= lo[b] <= x[b] <= hi[b] <= len(seqs[int(seq[b])])
    assert np.abs(qtable).max() <= 2 ** 31
    return rref.refine(seqs, kmer_length, qtable, seq, lo, x, hi, left_row, right_row, symbols.decode("latin-1"))


@pytest.fixture
def compose(monkeypatch):
    from phamers_amd import compose as cp
    from phamers_amd import refine
    from tests import compose_groups_ref as gref
    monkeypatch.setattr(cp, "_estep", cref.StatementEStep)
    monkeypatch.setattr(cp, "_estep_groups", gref.StatementGroupEStep)
    monkeypatch.setattr(refine, "_refine", _statement)
    return cp


# ---- boundary_plan ----------------------------------------------------------------------------------------------------------
def _decode(run_lengths_per_record, step):
    """(state, owner, start) of records whose runs have the given lengths in windows, states 0, 1, 2, 0, ... per record."""
    state, owner, start = [], [], []
    for r, runs in enumerate(run_lengths_per_record):
        t = 0
        for i, n in enumerate(runs):
            for _ in range(n):
                state.append((i + r) % 3)
                owner.append(r)
                start.append(t * step)
                t += 1
    return np.array(state), np.array(owner), np.array(start)


RUNS = [[1, 1, 2, 1, 40, 2, 2, 7, 1], [5], [1, 3], [], [30, 1, 30], [2, 2]]
PLANS = [(500, 500, None), (500, 500, 100), (500, 500, 5000), (500, 250, None), (500, 250, 60), (500, 125, 3000), (6, 4, None),
         (500, 800, None), (500, 800, 2000), (10, 30, 3), (7, 2, None), (2, 2, None), (500, 500, 0)]


@pytest.mark.parametrize("window,step,span", PLANS)
def test_boundary_plan_equals_the_loop(window, step, span):
    from phamers_amd import compose
    state, owner, start = _decode(RUNS, step)
    got = compose.boundary_plan(state, owner, start, window, step, span)
    want = rref.boundary_plan(state, owner, start, window, step, span)
    assert got._fields == ("record", "x", "lo", "hi", "left_state", "right_state", "first_window")
    for name, g, w in zip(got._fields, got, want):
        assert g.dtype == np.int64 and np.array_equal(g, np.array(w, dtype=np.int64)), name
    n_runs = [len(r) for r in RUNS]
    assert len(got.x) == sum(max(n - 1, 0) for n in n_runs)                 # one per adjacent pair, none across records
    assert np.array_equal(np.bincount(got.record, minlength=len(RUNS)), [max(n - 1, 0) for n in n_runs])
    if window == step:
        assert np.array_equal(got.x, start[got.first_window])
    assert (got.lo <= got.x).all() and (got.x <= got.hi).all() and (got.lo >= 0).all()
    assert (got.hi - got.lo <= 2 * (window if span is None else span)).all()
    last = np.array([start[owner == r].max() + window if (owner == r).any() else 0 for r in range(len(RUNS))])
    assert (got.hi <= last[got.record]).all()
    # disjoint and ordered: within a record every interval ends below the start of the next
    same = got.record[1:] == got.record[:-1]
    assert (got.hi[:-1][same] < got.lo[1:][same]).all()


def test_boundary_plan_edges():
    from phamers_amd import compose
    empty = compose.boundary_plan([], [], [], 500, 500)
    assert all(len(v) == 0 and v.dtype == np.int64 for v in empty)
    one = compose.boundary_plan([0, 0, 0], [0, 0, 0], [0, 500, 1000], 500, 500)
    assert len(one.x) == 0
    # the same state on either side of a record change is no boundary
    two = compose.boundary_plan([0, 1, 1, 0], [0, 0, 1, 1], [0, 500, 0, 500], 500, 500)
    assert two.record.tolist() == [0, 1] and two.x.tolist() == [500, 500]
    assert two.lo.tolist() == [251, 251] and two.hi.tolist() == [750, 750]
    for bad in (dict(window=0, step=1), dict(window=1, step=0), dict(window=5, step=5, span=-1)):
        with pytest.raises(ValueError):
            compose.boundary_plan([0, 1], [0, 0], [0, 5], **bad)
    with pytest.raises(ValueError):
        compose.boundary_plan([0, 1], [0], [0, 5], 5, 5)


# ---- refine.boundaries: arguments -----------------------------------------------------------------------------------------
def test_boundaries_and_argument_errors(compose):
    from phamers_amd import refine, segment
    rng = np.random.default_rng(5)
    seqs = ["".join("ATGC"[d] for d in rng.integers(0, 4, 300)), "ACGTNACGTTTGACCA"]
    logp = np.log(rng.dirichlet(np.ones(16), 3))
    args = dict(seq=[0, 1, 0], lo=[10, 0, 50], x=[100, 8, 50], hi=[250, 16, 50], left_row=[0, 1, 2], right_row=[1, 2, 0])
    got = refine.boundaries(seqs, 2, logp, **args)
    pos, ev, sup = rref.refine(seqs, 2, segment.quantise(logp), **args)
    assert np.array_equal(got.position, pos) and np.array_equal(got.support, sup)
    assert np.array_equal(np.stack([got.gain, got.left_evidence, got.right_evidence], axis=1), ev)
    assert got.position.dtype == got.gain.dtype == got.support.dtype == np.int64
    assert np.array_equal(got.gain_nats, ev[:, 0] * 2.0 ** -16) and np.array_equal(got.right_evidence_nats, ev[:, 2] * 2.0 ** -16)
    assert (ev >= 0).all() and got.position[2] == 50 and sup[2] == 0 and not ev[2].any()
    none = refine.boundaries(seqs, 2, logp, [], [], [], [], [], [])
    assert len(none.position) == 0 and none.gain_nats.shape == (0,)

    def bad(**change):
        a = dict(args)
        k, lp = change.pop("k", 2), change.pop("logp", logp)
        a.update(change)
        with pytest.raises(ValueError):
            refine.boundaries(seqs, k, lp, **a)
    bad(k=3)                                        # D is not 4^k
    bad(k=0)
    bad(k=8, logp=np.zeros((1, 4)))
    bad(logp=logp[0])
    bad(logp=np.where(np.arange(16) == 3, np.nan, logp))
    bad(left_row=[0, 1, 3])
    bad(right_row=[-1, 1, 2])
    bad(lo=[101, 0, 50])                            # lo > x
    bad(hi=[99, 16, 50])                            # x > hi
    bad(lo=[10, 0])
    bad(x=[100.0, 8.0, 50.0])
    bad(seq=[[0, 1, 0]])
    bad(lo=[0, 0, 50], x=[5, 8, 50], hi=[2 ** 30 + 1, 16, 50])
    with pytest.raises(NotImplementedError):
        refine.boundaries(seqs, 2, logp, symbols="ACGTN", **args)


# ---- refined_regions, segment_sequences(refine=) and the command line ----------------------------------------------------
def _two_records():
    from tests import segment_ref
    rows = cref.small_rows()
    return [cref.small_sequence(2),
            segment_ref.chain_sequence(np.random.default_rng(21), rows[1:3], [0, 15230, 30000], 30000), "ACGT" * 1500]


def _fasta(tmp_path, seqs):
    path = str(tmp_path / "in.fasta")
    with open(path, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">rec%d some words\n%s\n" % (i, s))
    return path


def _check_refined(result, seqs, span):
    """``boundaries`` and ``refined_regions`` of ``result`` against the statement applied to its decode."""
    from phamers_amd import compose, segment
    plan = rref.boundary_plan(result.state, result.owner, result.start, result.window, result.step, span)
    rec, x, lo, hi, ls, rs, _ = plan
    comp = result.composition
    if isinstance(comp, compose.Compositions):
        S = comp.n_states
        q = segment.quantise(np.where(np.isnan(comp.log_profiles), 0.0, comp.log_profiles).reshape(-1, comp.n_columns))
        left, right = [r * S + s for r, s in zip(rec, ls)], [r * S + s for r, s in zip(rec, rs)]
    else:
        q, left, right = segment.quantise(comp.log_profiles), ls, rs
    pos, ev, sup = rref.refine(seqs, 4, q, rec, lo, x, hi, left, right)
    b = result.boundaries
    assert np.array_equal(b.record, rec) and np.array_equal(b.window_boundary, x) and np.array_equal(b.position, pos)
    assert np.array_equal(b.left_state, ls) and np.array_equal(b.right_state, rs) and np.array_equal(b.support, sup)
    assert np.array_equal(b.evidence_q, ev) and np.array_equal(b.gain, ev[:, 0] * 2.0 ** -16)
    assert np.array_equal(b.left_evidence, ev[:, 1] * 2.0 ** -16) and np.array_equal(b.right_evidence, ev[:, 2] * 2.0 ** -16)
    assert b.record_id == [result.record_ids[r] for r in rec]
    # refined_regions: regions() with the interior ends moved
    plain, fine = result.regions(), result.refined_regions()
    assert len(plain) == len(fine) and len(pos) == sum(1 for p, n in zip(plain[:-1], plain[1:]) if p[0] == n[0])
    j = 0
    for i, (p, f) in enumerate(zip(plain, fine)):
        assert f[0] == p[0] and repr(f[3:]) == repr(p[3:])                    # (repr: the mean posterior of an unfitted record is NaN)
        first = i == 0 or plain[i - 1][0] != p[0]
        last = i + 1 == len(plain) or plain[i + 1][0] != p[0]
        assert f[1] == (p[1] if first else int(pos[j - 1]))
        assert f[2] == (p[2] if last else int(pos[j]))
        assert f[1] < f[2]                                                 # no refined region is empty or out of order
        j += 0 if last else 1
    assert j == len(pos)
    return pos


def test_segment_sequences_refine_and_refined_regions(compose, tmp_path):
    seqs = _two_records()
    path, d = _fasta(tmp_path, seqs), str(tmp_path / "out")
    host = _segment_on_the_host(compose)

    def segment(n_states, refine=False, **options):
        """``segment_sequences``' last lines over the host's window counter (the device's is not here)."""
        result = host(path, n_states, **options)
        refine, span = compose._span(refine)
        return result.refine(seqs, span) if refine else result

    plain = segment(3, max_iter=3)
    assert plain.boundaries is None
    with pytest.raises(ValueError):
        plain.refined_regions()
    with pytest.raises(ValueError):
        compose.write_refined_files(d, plain)
    whole = segment(3, refine=True, max_iter=3)
    pos = _check_refined(whole, seqs, None)
    assert len(pos) >= 2 and (pos != whole.boundaries.window_boundary).any()
    assert np.array_equal(whole.state, plain.state) and whole.regions() == plain.regions()
    narrow = segment(3, refine=40, max_iter=3)
    _check_refined(narrow, seqs, 40)
    assert (np.abs(narrow.boundaries.position - narrow.boundaries.window_boundary) <= 40).all()
    still = segment(3, refine=0, max_iter=3)                               # span 0: every boundary stays on the grid
    assert np.array_equal(still.boundaries.position, still.boundaries.window_boundary)
    assert still.refined_regions() == still.regions()
    # from the file instead of the strings: the same
    again = plain.refine(path)
    assert again is plain and np.array_equal(plain.boundaries.position, whole.boundaries.position)
    # one chain per record: rows g S + s; the record that was not fitted has no boundary
    per = segment(2, refine=True, per_record=True, max_iter=3)
    assert per.composition.status.tolist() == [0, 0, 1]
    _check_refined(per, seqs, None)
    assert 2 not in per.boundaries.record.tolist()
    for bad in (-1, 2.5, "yes"):
        with pytest.raises(ValueError):
            compose._span(bad)
    assert compose._span(False) == (False, None) and compose._span(None) == (False, None)
    assert compose._span(True) == (True, None) and compose._span(0) == (True, 0) and compose._span(300) == (True, 300)


def test_segment_sequences_takes_refine():
    """The public signature: ``refine`` is a keyword of ``segment_sequences`` and is checked before any device work."""
    import inspect
    from phamers_amd import compose
    assert inspect.signature(compose.segment_sequences).parameters["refine"].default is False
    with pytest.raises(ValueError):
        compose.segment_sequences(["ACGT" * 500], 2, refine=-5)


def test_command_line_files(compose, tmp_path, monkeypatch):
    monkeypatch.setattr(compose, "segment_sequences", _segment_on_the_host(compose))
    seqs = _two_records()
    fasta = _fasta(tmp_path, seqs)
    four = ["compose_profiles.csv", "compose_segments.csv", "compose_trace.csv", "compose_windows.csv"]
    # without the flag: byte for byte the old directory
    old_dir = str(tmp_path / "old")
    result = compose.main(["-in", fasta, "-out", old_dir, "-S", "3", "--max_iter", "3"])
    assert sorted(os.listdir(old_dir)) == four and result.boundaries is None
    for name, text in _old_files(old_dir, result).items():
        assert open(os.path.join(old_dir, name)).read() == text, name
    # with it: the same four files, byte for byte, and two more
    new_dir = str(tmp_path / "new")
    refined = compose.main(["-in", fasta, "-out", new_dir, "-S", "3", "--max_iter", "3", "--refine"])
    assert sorted(os.listdir(new_dir)) == sorted(four + ["compose_boundaries.csv", "compose_segments_refined.csv"])
    for name in four:
        assert open(os.path.join(new_dir, name)).read() == open(os.path.join(old_dir, name)).read(), name
    _check_refined(refined, seqs, None)
    b = refined.boundaries
    lines = open(os.path.join(new_dir, "compose_boundaries.csv")).read().splitlines()
    assert lines[0] == "record_id,window_boundary,position,left_state,right_state,gain,left_evidence,right_evidence,support"
    assert len(lines) == 1 + len(b.position) and len(b.position) >= 2
    for i, line in enumerate(lines[1:]):
        assert line == "%s,%d,%d,%d,%d,%r,%r,%r,%d" % (b.record_id[i], b.window_boundary[i], b.position[i], b.left_state[i],
                                                       b.right_state[i], float(b.gain[i]), float(b.left_evidence[i]),
                                                       float(b.right_evidence[i]), b.support[i])
    seg = open(os.path.join(new_dir, "compose_segments_refined.csv")).read()
    assert seg == "record_id,start,end,state,n_windows,mean_posterior\n" + "".join("%s,%d,%d,%d,%d,%r\n" % r
                                                                                 for r in refined.refined_regions())
    # --refine SPAN
    span_dir = str(tmp_path / "span")
    spanned = compose.main(["-in", fasta, "-out", span_dir, "-S", "3", "--max_iter", "3", "--refine", "30"])
    _check_refined(spanned, seqs, 30)
    assert (np.abs(spanned.boundaries.position - spanned.boundaries.window_boundary) <= 30).all()
    with pytest.raises(SystemExit):
        compose.main(["-in", fasta, "-out", span_dir, "-S", "3", "--refine", "-3"])
    # --per_record: without the flag the five files of before, with it two more
    rec_dir, rec_new = str(tmp_path / "rec"), str(tmp_path / "rec_refined")
    compose.main(["-in", fasta, "-out", rec_dir, "-S", "2", "--max_iter", "3", "--per_record"])
    per = compose.main(["-in", fasta, "-out", rec_new, "-S", "2", "--max_iter", "3", "--per_record", "--refine"])
    five = sorted(four + ["compose_records.csv"])
    assert sorted(os.listdir(rec_dir)) == five
    assert sorted(os.listdir(rec_new)) == sorted(five + ["compose_boundaries.csv", "compose_segments_refined.csv"])
    for name in five:
        assert open(os.path.join(rec_new, name)).read() == open(os.path.join(rec_dir, name)).read(), name
    _check_refined(per, seqs, None)
    assert len(per.boundaries.position) >= 1
