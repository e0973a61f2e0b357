"""CPU-only: ``compose.fit_groups`` driven by the statement of the grouped E-step
(tests/compose_groups_ref.py) in the place of the device equals, bit for bit, the loop of ``compose.fit`` per group driven by
the statement of the single chain; a group that stops early leaves the others' bits alone and drops out of the later
calls; save / load_groups; argument errors; the files of the command line with and without --per_record."""
import os

import numpy as np
import pytest

from tests import compose_groups_ref as gref
from tests import compose_ref as cref


@pytest.fixture
def compose(monkeypatch):
    from phamers_amd import compose as cp
    monkeypatch.setattr(cp, "_estep", cref.StatementEStep)
    monkeypatch.setattr(cp, "_estep_groups", gref.StatementGroupEStep)
    gref.StatementGroupEStep.calls = []
    return cp


@pytest.fixture(scope="module")
def assembly():
    """Six groups over seven records: three "small" sequences of different seeds, one scaffold of a single composition (two
    records), one too short for S = 3 (30 windows: two blocks of 20), one without records."""
    from tests import segment_ref
    small = [cref.window_counts(cref.small_sequence(seed)) for seed in (2, 3, 4)]
    rows = cref.small_rows()
    single = cref.window_counts(segment_ref.chain_sequence(np.random.default_rng(11), rows[:1], [0, 35000], 35000))
    short = cref.window_counts(segment_ref.chain_sequence(np.random.default_rng(12), rows[1:3], [0, 8000, 15000], 15000))
    parts = small + [single[:45], single[45:], short]
    counts = np.vstack(parts)
    offsets = np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.uint64)
    group_offsets = np.array([0, 1, 2, 3, 5, 5, 6], dtype=np.uint64)      # group 4 holds no record
    return counts, offsets, group_offsets


def test_fit_groups_equals_the_loop_of_fit(compose, assembly):
    counts, offsets, go = assembly
    got = compose.fit_groups(counts, offsets, go, 3)
    want, status = gref.fit_loop(compose, counts, offsets, go, 3)
    assert status.tolist() == [0, 0, 0, 0, 1, 1] and np.array_equal(got.status, status)
    assert compose.GROUP_FITTED == gref.GROUP_FITTED == 0 and compose.GROUP_TOO_SHORT == gref.GROUP_TOO_SHORT == 1
    assert len(got) == 6
    for g in range(6):
        gref.assert_same_composition(got[g], want[g], "group %d" % g)
    # the stacked arrays are the compositions', NaN where a group was not fitted
    for g in range(4):
        for name in ("log_profiles", "trans", "init", "occupancy", "expected_counts"):
            assert np.array_equal(getattr(got, name)[g], getattr(want[g], name)), (g, name)
        assert np.array_equal(got.traces[g], want[g].trace)
        assert (got.n_iter[g], got.converged[g], got.bic[g]) == (want[g].n_iter, want[g].converged, want[g].bic)
    for g in (4, 5):
        assert got[g] is None and np.isnan(got.log_profiles[g]).all() and np.isnan(got.trans[g]).all()
        assert np.isnan(got.bic[g]) and got.n_iter[g] == 0 and not got.converged[g] and got.traces[g].shape == (0, 2)
    assert got.log_profiles.shape == (6, 3, 256) and got.trans.shape == (6, 3, 3) and got.init.shape == (6, 3)
    # the groups stop at different iterations; one that has stopped is inactive in every later call, and the groups that
    # were never fitted are inactive from the first
    n_calls = [int(got.n_iter[g]) + 1 for g in range(4)]
    assert len(set(n_calls)) > 1, n_calls
    calls = gref.StatementGroupEStep.calls
    assert len(calls) == max(n_calls)
    for i, active in enumerate(calls):
        assert active.tolist() == [i < n_calls[g] for g in range(4)] + [False, False], (i, active)
    # the decode: the loop of Composition.decode; the groups that were not fitted get state 0 and NaN
    dec = compose.Compositions.decode(got, counts, offsets, go)
    off = [int(o) for o in offsets]
    for g, (r0, r1, w0, w1) in enumerate(gref.group_spans(offsets, go)):
        if want[g] is None:
            assert not dec.state[w0:w1].any() and np.isnan(dec.posterior[w0:w1]).all() and np.isnan(dec.log_evidence[r0:r1]).all()
            continue
        rows, roff = gref.group_rows(counts, offsets, go, g)
        alone = want[g].decode(rows, roff)
        assert np.array_equal(dec.state[w0:w1], alone.state) and np.array_equal(dec.posterior[w0:w1], alone.posterior)
        assert np.array_equal(dec.log_evidence[r0:r1], alone.log_evidence)
        assert np.array_equal(dec.path_score_q[r0:r1], alone.path_score_q) and np.array_equal(dec.path_score[r0:r1], alone.path_score)
    assert cref.changes(dec.state[off[0]:off[1]]) == [12000, 20000, 30000]


def test_a_group_that_stops_early_leaves_the_others_alone(compose, assembly):
    counts, offsets, go = assembly
    every = compose.fit_groups(counts, offsets, go, 3)
    # groups 0 and 3 alone, as a call of two groups: the same bits as inside the call of six
    sub_counts = np.vstack([counts[int(offsets[0]):int(offsets[1])], counts[int(offsets[3]):int(offsets[5])]])
    n0, n3a, n3b = int(offsets[1]), int(offsets[4] - offsets[3]), int(offsets[5] - offsets[4])
    sub = compose.fit_groups(sub_counts, [0, n0, n0 + n3a, n0 + n3a + n3b], [0, 1, 3], 3)
    gref.assert_same_composition(sub[0], every[0], "group 0")
    gref.assert_same_composition(sub[1], every[3], "group 3")
    assert every.n_iter[0] != every.n_iter[3]
    # max_iter cuts every group at the same iterate; the options reach every group
    cut = compose.fit_groups(counts, offsets, go, 3, max_iter=1, fit_transitions=False, p_start='free', block=8)
    want, status = gref.fit_loop(compose, counts, offsets, go, 3, block=8, max_iter=1, fit_transitions=False, p_start='free')
    assert np.array_equal(cut.status, status)
    for g in range(6):
        gref.assert_same_composition(cut[g], want[g], "group %d" % g)
    # init per group: block indices for one group, profiles for another, the start rule for the rest
    init = [None, np.array([0, 1, 2]), None, np.exp(every[3].log_profiles), None, None]
    mixed = compose.fit_groups(counts, offsets, go, 3, init=init, max_iter=2)
    want, _ = gref.fit_loop(compose, counts, offsets, go, 3, init=init, max_iter=2)
    for g in range(6):
        gref.assert_same_composition(mixed[g], want[g], "group %d" % g)


def test_save_load_and_label(compose, assembly, tmp_path, monkeypatch):
    counts, offsets, go = assembly
    fitted = compose.fit_groups(counts, offsets, go, 3, max_iter=2)
    path = str(tmp_path / "groups.npz")
    fitted.save(path)
    back = compose.load_groups(path)
    assert len(back) == len(fitted) and np.array_equal(back.status, fitted.status)
    for g in range(len(fitted)):
        gref.assert_same_composition(back[g], fitted[g], "group %d" % g)
    for name in ("log_profiles", "trans", "init", "occupancy", "expected_counts", "bic"):
        assert np.array_equal(getattr(back, name), getattr(fitted, name), equal_nan=True), name
    assert np.array_equal(back.n_iter, fitted.n_iter) and np.array_equal(back.converged, fitted.converged)
    assert (back.temper, back.pseudocount, back.n_states, back.n_columns) == (fitted.temper, fitted.pseudocount, 3, 256)
    # label: (G, S), every fitted group's Composition.label, NaN for the others
    from phamers_amd import likelihood
    monkeypatch.setattr(likelihood, "score", lambda rows, p, n, pseudocount=0.5, per_kmer=False:
                        np.asarray(rows, dtype=np.float64).sum(axis=1) * 2.0 ** -10)
    label = fitted.label(None, None)
    assert label.shape == (6, 3) and np.isnan(label[4:]).all()
    for g in range(4):
        assert np.array_equal(label[g], fitted[g].label(None, None))


def test_argument_errors(compose, assembly):
    counts, offsets, go = assembly
    with pytest.raises(ValueError):
        compose.fit_groups(counts, offsets, go, 3, scan=True)
    with pytest.raises(ValueError):
        compose.fit_groups(counts, offsets, go, 3, scan=None)           # the argument itself is refused
    with pytest.raises(TypeError):
        compose.fit_groups(counts, offsets, go, 3, no_such_option=1)
    for bad in ([0, 1, 2], [1, 7], [0, 3, 2, 7], [[0, 7]], [0.0, 7.0], []):
        with pytest.raises(ValueError):
            compose.fit_groups(counts, offsets, bad, 3)
    for bad in (dict(n_states=1), dict(n_states=9), dict(n_states=3, temper=0.0), dict(n_states=3, pseudocount=0.0),
                dict(n_states=3, p_start='other'), dict(n_states=3, max_iter=-1), dict(n_states=3, init=[None] * 5),
                dict(n_states=3, init=[np.array([0, 1])] + [None] * 5)):
        with pytest.raises(ValueError):
            compose.fit_groups(counts, offsets, go, **bad)
    fitted = compose.fit_groups(counts, offsets, go, 3, max_iter=0)
    with pytest.raises(ValueError):
        fitted.decode(counts, offsets, [0, 7])                             # one group, six compositions
    with pytest.raises(ValueError):
        fitted.decode(counts[:, :64], offsets, go)
    with pytest.raises(ValueError):
        compose.segment_sequences(["ACGT" * 500], 2, scan=True, per_record=True)


# ---- the command line ------------------------------------------------------------------------------------------------------
def _segment_on_the_host(compose):
    """``segment_sequences`` without the device's window counter: the sequences of a FASTA file counted by the statement."""
    def segment(fasta, n_states, window=500, step=500, kmer_length=4, both_strands=False, scan=None, per_record=False,
                **options):
        ids, seqs = [], []
        for line in open(fasta):
            if line.startswith(">"):
                ids.append(line[1:].split()[0])
                seqs.append("")
            else:
                seqs[-1] += line.strip()
        parts = [cref.window_counts(s, window, kmer_length) for s in seqs]
        counts = np.vstack(parts)
        lens = [len(p) for p in parts]
        offsets = compose._KnownOffsets(np.concatenate(([0], np.cumsum(lens))))
        owner = np.repeat(np.arange(len(parts)), lens)
        first = np.concatenate([np.arange(n) * step for n in lens])
        if per_record:
            groups = np.arange(len(parts) + 1)
            comp = compose.fit_groups(counts, offsets, groups, n_states, step=step, **options)
            dec = comp.decode(counts, offsets, groups)
        else:
            comp = compose.fit(counts, offsets, n_states, step=step, **options)
            dec = comp.decode(counts, offsets)
        return compose.ComposedSequences(comp, ids, owner, first, window, step, dec)
    return segment


def _old_files(directory, result, phage_score=None):
    """The four files as the command line wrote them before --per_record existed, restated."""
    comp = result.composition
    S, D = comp.log_profiles.shape
    text = {}
    text["compose_windows.csv"] = "record_id,start,state," + ",".join("posterior%d" % s for s in range(S)) + "\n" + "".join(
        "%s,%d,%d,%s\n" % (result.record_ids[int(result.owner[i])], int(result.start[i]), int(result.state[i]),
                           ",".join(repr(float(v)) for v in result.posterior[i])) for i in range(len(result)))
    text["compose_segments.csv"] = "record_id,start,end,state,n_windows,mean_posterior\n" + "".join(
        "%s,%d,%d,%d,%d,%r\n" % r for r in result.regions())
    text["compose_profiles.csv"] = "state,occupancy,self_transition,mean_region," + ",".join("p%d" % j for j in range(D)) + "\n" + "".join(
        "%d,%r,%r,%r,%s\n" % (s, float(comp.occupancy[s]), float(comp.trans[s, s]), result.step / (1.0 - float(comp.trans[s, s])),
                              ",".join(repr(float(v)) for v in np.exp(comp.log_profiles[s]))) for s in range(S))
    text["compose_trace.csv"] = "iteration,L,F\n" + "".join("%d,%r,%r\n" % (i, float(L), float(F))
                                                            for i, (L, F) in enumerate(comp.trace))
    return text


def test_command_line_files(compose, tmp_path, monkeypatch):
    from tests import segment_ref
    monkeypatch.setattr(compose, "segment_sequences", _segment_on_the_host(compose))
    rows = cref.small_rows()
    seqs = [cref.small_sequence(2), segment_ref.chain_sequence(np.random.default_rng(21), rows[1:3], [0, 15000, 30000], 30000),
            "ACGT" * 1500]                                                 # the last: 12 windows, too short for two blocks of 20
    fasta = str(tmp_path / "in.fasta")
    with open(fasta, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">rec%d some words\n%s\n" % (i, s))
    # without the flag: the four files, byte for byte the old ones
    old_dir = str(tmp_path / "old")
    result = compose.main(["-in", fasta, "-out", old_dir, "-S", "2", "--max_iter", "3"])
    assert sorted(os.listdir(old_dir)) == ["compose_profiles.csv", "compose_segments.csv", "compose_trace.csv", "compose_windows.csv"]
    for name, text in _old_files(old_dir, result).items():
        assert open(os.path.join(old_dir, name)).read() == text, name
    # with it: record_id leads the profiles and the trace, and compose_records.csv is there
    new_dir = str(tmp_path / "new")
    result = compose.main(["-in", fasta, "-out", new_dir, "-S", "2", "--max_iter", "3", "--per_record"])
    comps = result.composition
    assert isinstance(comps, compose.Compositions) and comps.status.tolist() == [0, 0, 1]
    assert sorted(os.listdir(new_dir)) == ["compose_profiles.csv", "compose_records.csv", "compose_segments.csv",
                                           "compose_trace.csv", "compose_windows.csv"]
    lines = lambda name: open(os.path.join(new_dir, name)).read().splitlines()
    prof = lines("compose_profiles.csv")
    assert prof[0].startswith("record_id,state,occupancy,self_transition,mean_region,p0,") and len(prof) == 1 + 2 * 2
    assert [l.split(",")[:2] for l in prof[1:]] == [["rec0", "0"], ["rec0", "1"], ["rec1", "0"], ["rec1", "1"]]
    assert float(prof[3].split(",")[2]) == float(comps[1].occupancy[0])
    trace = lines("compose_trace.csv")
    assert trace[0] == "record_id,iteration,L,F" and len(trace) == 1 + sum(len(t) for t in comps.traces)
    assert trace[1] == "rec0,0,%r,%r" % (float(comps.traces[0][0, 0]), float(comps.traces[0][0, 1]))
    rec = lines("compose_records.csv")
    assert rec[0] == "record_id,n_windows,status,n_iter,converged,log_evidence,bic" and len(rec) == 4
    assert rec[1] == "rec0,80,0,%d,%d,%r,%r" % (comps.n_iter[0], comps.converged[0], float(result.log_evidence[0]), float(comps.bic[0]))
    assert rec[3] == "rec2,12,1,0,0,nan,nan"
    assert len(lines("compose_windows.csv")) == 1 + 80 + 60 + 12
    # the phage score is per (record, state)
    from phamers_amd import fileIO
    monkeypatch.setattr(fileIO, "read_feature_file", lambda path, normalize=False: (None, None))
    monkeypatch.setattr(compose.Compositions, "label", lambda self, p, n: np.arange(6, dtype=np.float64).reshape(3, 2))
    scored = str(tmp_path / "scored")
    compose.main(["-in", fasta, "-out", scored, "-S", "2", "--max_iter", "1", "--per_record", "-pf", "p", "-nf", "n"])
    prof = open(os.path.join(scored, "compose_profiles.csv")).read().splitlines()
    assert prof[0].split(",")[:6] == ["record_id", "state", "occupancy", "self_transition", "mean_region", "phage_score"]
    assert [l.split(",")[5] for l in prof[1:]] == ["0.0", "1.0", "2.0", "3.0"]
    with pytest.raises(SystemExit):
        compose.main(["-in", fasta, "-out", scored, "-S", "2", "--per_record", "--scan"])
