"""GPU: the two-state hidden Markov decode (csrc/segment.hip, phamers_amd/segment.py) and the likelihood window tracks
(phamers_amd/windows.py) against the statements of tests/segment_ref.py: the Viterbi path and its score equal to the integer
recurrence (i), the posterior and log_odds within the derived bound (iv) of the longdouble statement (ii), and a record's
outputs -- the float ones too -- bit for bit the same whatever else the call holds.  T = PHK_SEG_TILE = 64."""
import numpy as np
import pytest

from tests import helpers, segment_ref as ref

pytestmark = pytest.mark.gpu

T = 64
A, B = 0.05, 0.1
LENGTHS = [1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, 64 * T - 1, 64 * T, 64 * T + 1]


def length_case(n):
    return ref.biased_evidence(np.random.default_rng(100 + n), n)


def ragged_case(records=300, seed=7):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 5 * T + 1, records)
    lengths[[0, 10, 11, records - 1]] = 0            # empty records first, adjacent and last
    lengths[[1, 2, 3, 4]] = [T, 5 * T, 1, T + 1]
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    return ref.biased_evidence(rng, int(off[-1])), off


def owners(n):
    """One record of n windows, as ``segment.decode`` takes it: the owner of every window ((n,) entries are owners), or
    the offsets of a record without windows."""
    return np.zeros(n, dtype=np.int64) if n else [0, 0]


def quantised(a, b, s=None):
    from phamers_amd import segment
    return segment.parameters(a, b, s)


def check_viterbi(d, x, off, a, b, s=None, records=None):
    trans, init, qt, qp = quantised(a, b, s)
    for r in (range(len(off) - 1) if records is None else records):
        lo, hi = int(off[r]), int(off[r + 1])
        states, score = ref.viterbi(ref.quantise(x[lo:hi]) if hi > lo else [], qt, qp)
        assert np.array_equal(d.state[lo:hi], states), r
        assert int(d.path_score_q[r]) == score and d.path_score[r] == score * 2.0 ** -16, r


def same(d, e):
    return all(np.array_equal(u, v) for u, v in zip(d, e))


# ---- 1. record lengths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_one_record_against_both_statements(n):
    from phamers_amd import segment
    x = length_case(n)
    d = segment.decode(x, owners(n), A, B)
    assert d.posterior.dtype == np.float64 and d.state.dtype == np.uint8 and d.path_score_q.dtype == np.int64
    assert d.posterior.shape == d.state.shape == (n,) and d.log_odds.shape == d.path_score.shape == (1,)
    check_viterbi(d, x, [0, n], A, B)
    if n >= 2 * T:
        assert 0 < d.state.sum() < n                 # (the biased runs make the path switch)
    trans, init, _, _ = quantised(A, B)
    ref.check(d.posterior, d.log_odds[0], x, trans, init, what="n=%d" % n)
    # a start distribution and a temper of the caller's
    d = segment.decode(x, owners(n), A, B, p_start=0.5, temper=0.25)
    check_viterbi(d, 0.25 * x, [0, n], A, B, 0.5)
    trans, init, _, _ = quantised(A, B, 0.5)
    ref.check(d.posterior, d.log_odds[0], 0.25 * x, trans, init, what="tempered n=%d" % n)


# ---- 2. ragged calls -------------------------------------------------------------------------------------------------------
def test_ragged_records_equal_each_record_alone_in_any_order_and_run():
    from phamers_amd import segment
    x, off = ragged_case()
    R = len(off) - 1
    d = segment.decode(x, off, A, B)
    assert same(d, segment.decode(x, off, A, B))                      # run to run
    check_viterbi(d, x, off, A, B)
    trans, init, _, _ = quantised(A, B)
    for r in (1, 2, 3, 4, 150):
        ref.check(d.posterior[int(off[r]):int(off[r + 1])], d.log_odds[r], x[int(off[r]):int(off[r + 1])], trans, init)
    for r in range(R):
        lo, hi = int(off[r]), int(off[r + 1])
        one = segment.decode(x[lo:hi], owners(hi - lo), A, B)
        assert np.array_equal(one.posterior, d.posterior[lo:hi]) and np.array_equal(one.state, d.state[lo:hi]), r
        assert one.log_odds[0] == d.log_odds[r] and one.path_score_q[0] == d.path_score_q[r], r
        if hi == lo:
            assert d.log_odds[r] == 0.0 and d.path_score_q[r] == 0
    # the records in reversed order
    pieces = [x[int(off[r]):int(off[r + 1])] for r in range(R)][::-1]
    roff = np.concatenate(([0], np.cumsum([len(p) for p in pieces]))).astype(np.uint64)
    e = segment.decode(np.concatenate(pieces), roff, A, B)
    assert np.array_equal(e.log_odds, d.log_odds[::-1]) and np.array_equal(e.path_score_q, d.path_score_q[::-1])
    for r in range(R):
        lo, hi, s = int(off[r]), int(off[r + 1]), int(roff[R - 1 - r])
        assert np.array_equal(e.posterior[s:s + hi - lo], d.posterior[lo:hi]), r
        assert np.array_equal(e.state[s:s + hi - lo], d.state[lo:hi]), r


def test_more_tiles_than_one_grid_pass():
    """A call of more tiles than one launch covers equals the same records decoded in calls that stay below it, and a
    sample of its records -- the last ones, past the pass, among them -- equals each decoded alone and statement (i)."""
    from phamers_amd import _lib, segment
    grid_pass = int(_lib.load().phk_segment_grid_pass())
    assert grid_pass % T == 0
    rng = np.random.default_rng(11)
    R = grid_pass // 2
    lengths = rng.integers(0, 5 * T + 1, R)
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    tiles = int(((lengths + T - 1) // T).sum())
    assert tiles > grid_pass + 64 * T
    x = ref.biased_evidence(rng, int(off[-1]))
    d = segment.decode(x, off, A, B)
    assert np.isfinite(d.posterior).all() and np.isfinite(d.log_odds).all() and d.state.max() == 1
    cuts = np.linspace(0, R, 5).astype(int)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        a, b = int(off[lo]), int(off[hi])
        part = segment.decode(x[a:b], off[lo:hi + 1] - off[lo], A, B)
        assert np.array_equal(part.posterior, d.posterior[a:b]) and np.array_equal(part.state, d.state[a:b])
        assert np.array_equal(part.log_odds, d.log_odds[lo:hi]) and np.array_equal(part.path_score_q, d.path_score_q[lo:hi])
    sample = sorted(set(rng.integers(0, R, 24).tolist()) | set(range(R - 8, R)))
    check_viterbi(d, x, off, A, B, records=sample)
    for r in sample:
        lo, hi = int(off[r]), int(off[r + 1])
        one = segment.decode(x[lo:hi], owners(hi - lo), A, B)
        assert np.array_equal(one.posterior, d.posterior[lo:hi]) and one.log_odds[0] == d.log_odds[r], r


# ---- 3. extremes -----------------------------------------------------------------------------------------------------------
def extreme_cases(n=3 * T + 5):
    rng = np.random.default_rng(5)
    flip = np.repeat(rng.choice([-1.0, 1.0], n // 9 + 1), 9)[:n]
    return {"zero": np.zeros(n), "+800": np.full(n, 800.0), "-800": np.full(n, -800.0), "+-800": 800.0 * flip,
            "+-clamp*2": 2.0 ** 16 * flip, "clamp and beyond": np.where(np.arange(n) % 2 == 0, 2.0 ** 15, 2.0 ** 16) * flip}


@pytest.mark.parametrize("b", [1e-12, 0.5, 1 - 1e-12])
@pytest.mark.parametrize("a", [1e-12, 0.5, 1 - 1e-12])
def test_extreme_evidence_and_parameters(a, b):
    from phamers_amd import segment
    trans, init, _, _ = quantised(a, b)
    for name, x in extreme_cases().items():
        n = len(x)
        d = segment.decode(x, owners(n), a, b)
        assert np.isfinite(d.posterior).all() and np.isfinite(d.log_odds).all(), name
        assert (d.posterior >= 0).all() and (d.posterior <= 1).all() and d.state.max() <= 1, name
        check_viterbi(d, x, [0, n], a, b)
        want, _, _ = ref.check(d.posterior, d.log_odds[0], x, trans, init, what="%s a=%g b=%g" % (name, a, b))
        if name == "zero":
            # no evidence: the posterior is the prior chain's marginal pi A^t, and the evidence is that of the all-host chain
            Am, v, prior = np.asarray(trans, dtype=ref.LD).reshape(2, 2), np.asarray(init, dtype=ref.LD), []
            for _ in range(n):
                prior.append(v[1])
                v = v @ Am
            prior = np.array(prior)
            assert (np.abs(d.posterior.astype(ref.LD) - prior) <= ref.posterior_bound(n) * prior + ref.FLOOR).all()
            assert abs(d.log_odds[0]) <= ref.log_odds_bound(x, 0.0)


def test_exact_ties():
    from phamers_amd import segment
    n = 2 * T + 3
    # every step ties: the path is all 0
    d = segment.decode(np.zeros(n), owners(n), 0.5, 0.5)
    assert not d.state.any() and d.path_score_q[0] == n * int(quantised(0.5, 0.5)[2][0])
    # a = b = pi = 1/2: delta_t(1) - delta_t(0) is the step's own integer evidence, so a last x that quantises to 0 is a
    # tie at the final step -- it goes to state 0 -- and every x_t = 0 before a phage window ties between predecessors
    x = length_case(n)
    for last in (0.0, -0.0, 2.0 ** -17, -2.0 ** -17):               # (rint(+-1/2) = 0: ties to even)
        x[-1] = last
        x[T - 1:T + 2] = [0.0, 5.0, 0.0]
        d = segment.decode(x, owners(n), 0.5, 0.5)
        check_viterbi(d, x, [0, n], 0.5, 0.5)
        assert d.state[-1] == 0 and d.state[T - 1] == 0 and d.state[T] == 1
    x[-1] = 3 * 2.0 ** -17                                           # rint(3/2) = 2 > 0: no tie
    d = segment.decode(x, owners(n), 0.5, 0.5)
    check_viterbi(d, x, [0, n], 0.5, 0.5)
    assert d.state[-1] == 1


# ---- 4. error codes --------------------------------------------------------------------------------------------------------
def test_errors_before_any_launch():
    from phamers_amd import _lib, segment
    ctx = _lib.get_context()
    x = np.ones(5)
    trans, init, qt, qp = quantised(A, B)
    good = segment.decode(x, [0, 5], A, B)

    def rc(x=x, off=(0, 5), trans=trans, init=init):
        off = np.asarray(off, dtype=np.uint64)
        out = np.empty(len(x)), np.empty(len(x), dtype=np.uint8), np.empty(len(off) - 1), np.empty(len(off) - 1, dtype=np.int64)
        return ctx.lib.phk_segment_decode(ctx.handle, _lib.ptr(np.ascontiguousarray(x, dtype=np.float64)), len(x), _lib.ptr(off),
                                          len(off) - 1, _lib.ptr(np.ascontiguousarray(trans)), _lib.ptr(np.ascontiguousarray(init)),
                                          _lib.ptr(qt), _lib.ptr(qp), *[_lib.ptr(o) for o in out])
    assert rc() == _lib.PHK_OK
    for bad in ([0.0, 1.0, B, 1 - B], [1 - A, A, 1.0, 0.0], [1 - A, A + 1e-9, B, 1 - B], [1 - A, A, B, 1 - B - 1e-9],
                [np.nan, A, B, 1 - B], [1 + A, -A, B, 1 - B]):
        assert rc(trans=np.array(bad)) == _lib.PHK_ERR_ARG, bad
    for bad in ([0.0, 1.0], [0.5, 0.5 + 1e-9], [np.nan, 0.5]):
        assert rc(init=np.array(bad)) == _lib.PHK_ERR_ARG, bad
    for bad in ((1, 5), (0, 4), (0, 6), (0, 3, 2, 5)):
        assert rc(off=bad) == _lib.PHK_ERR_ARG, bad
    for bad in (np.inf, -np.inf):
        assert rc(x=np.array([1.0, bad, 1.0, 1.0, 1.0])) == _lib.PHK_ERR_NAN
    assert rc(x=np.zeros(0), off=(0,)) == _lib.PHK_OK and rc(x=np.zeros(0), off=(0, 0, 0)) == _lib.PHK_OK
    # the Python layer: ValueError, and nan scores are no evidence
    for a, b in ((0.0, B), (1.0, B), (A, 0.0), (A, 1.0), (np.nan, B), (1e-20, B)):
        with pytest.raises(ValueError):
            segment.decode(x, [0, 5], a, b)
    for kw in (dict(p_start=0.0), dict(p_start=1.0), dict(temper=0.0), dict(temper=np.inf)):
        with pytest.raises(ValueError):
            segment.decode(x, [0, 5], A, B, **kw)
    with pytest.raises(ValueError):
        segment.decode([1.0, np.inf], [0, 2], A, B)
    with pytest.raises(ValueError):
        segment.decode(x, [0, 3, 2, 5], A, B)
    with pytest.raises(ValueError):
        _lib.segment_decode(ctx, x, [1, 5], trans, init, qt, qp)
    empty = segment.decode(np.zeros(0), [0, 0, 0], A, B)
    assert empty.posterior.shape == (0,) and np.array_equal(empty.log_odds, [0.0, 0.0]) and not empty.path_score_q.any()
    with_nan = segment.decode([1.0, np.nan, 1.0, 1.0, 1.0], np.zeros(5, dtype=np.int64), A, B)
    assert same(with_nan, segment.decode([1.0, 0.0, 1.0, 1.0, 1.0], [0, 5], A, B))
    assert same(good, segment.decode(x, [0, 5], A, B))                # (the failed calls left nothing behind)


# ---- 5. likelihood tracks --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference():
    g = helpers.load_npz("ref_features.npz")
    return g["pos_counts"][:150].astype(np.int64), g["neg_counts"][:170].astype(np.int64)


def track_sequences():
    rng = np.random.default_rng(31)
    seqs = ["".join(rng.choice(list("ATGC"), L)) for L in (4000, 499, 3200, 2600)]
    s = list(seqs[2])
    s[1000:2100] = "N" * 1100                        # windows without a single valid k-mer
    seqs[2] = "".join(s)
    return seqs


@pytest.mark.parametrize("window,step", [(500, 500), (1000, 200)])
def test_likelihood_track_equals_scoring_the_window_rows(reference, window, step):
    from phamers_amd import kmer, likelihood, segment, windows
    pos, neg = reference
    seqs = track_sequences()
    track = windows.score_windows(seqs, pos, neg, window=window, step=step, kmer_length=4, method='likelihood')
    _, rows = kmer.count_windows(seqs, 4, window, step)
    details = {}
    want = likelihood.score(rows, pos, neg, _details=details)
    empty = rows.sum(axis=1) == 0
    assert empty.any() and not empty.all() and len(track) == len(rows)
    assert np.isnan(track.scores[empty]).all() and np.isnan(track.l_pos[empty]).all() and np.isnan(track.l_neg[empty]).all()
    assert track.l_pos.dtype == track.l_neg.dtype == np.float64
    assert np.array_equal(track.scores[~empty], want[~empty])
    assert np.array_equal(track.l_pos[~empty], details["l_pos"][~empty])
    assert np.array_equal(track.l_neg[~empty], details["l_neg"][~empty])
    assert np.array_equal(track.scores[~empty], (track.l_pos - track.l_neg)[~empty])
    assert track.positive_centroids is None and track.negative_centroids is None
    other = windows.score_windows(seqs, pos, neg, window=window, step=step, method='likelihood', pseudocount=2.0)
    assert not np.array_equal(other.scores[~empty], track.scores[~empty])
    # the run of N is no evidence for the chain, which carries across it
    seg = segment.segment_track(track)
    assert seg.temper == min(1.0, step / (window - 3.0)) and (seg.x[empty] == 0).all()
    assert np.array_equal(seg.x[~empty], seg.temper * track.scores[~empty])
    assert np.isfinite(seg.posterior).all() and len(seg.log_odds) == len(seqs) and seg.log_odds[1] == 0.0
    off = np.concatenate(([0], np.cumsum(np.bincount(track.owner, minlength=len(seqs)))))
    check_viterbi(segment.decode(track.scores, track.owner, seg.p_enter, seg.p_leave, temper=seg.temper), seg.x, off,
                  seg.p_enter, seg.p_leave)
    assert np.array_equal(segment.decode(track.scores, off, seg.p_enter, seg.p_leave, temper=seg.temper).state, seg.state)
    with pytest.raises(ValueError):                                   # frequencies are not counts
        windows.score_windows(seqs, pos / pos.sum(axis=1, keepdims=True), neg, window=window, step=step, method='likelihood')


def test_likelihood_track_of_the_reverse_complement_is_the_mirror(reference):
    from phamers_amd import transform_kmers, windows
    from tests import strands_ref
    pos, neg = (transform_kmers.fold_strands(c) for c in reference)
    rng = np.random.default_rng(32)
    for window, step in ((500, 500), (1000, 200)):
        seq = "".join(rng.choice(list("ATGC"), window + 11 * step))
        fwd = windows.score_windows([seq], pos, neg, window=window, step=step, method='likelihood', both_strands=True)
        rev = windows.score_windows([strands_ref.revcomp(seq)], pos, neg, window=window, step=step, method='likelihood',
                                    both_strands=True)
        assert len(fwd) == 12 and np.isfinite(fwd.scores).all()
        assert np.array_equal(fwd.scores, rev.scores[::-1])
        assert np.array_equal(fwd.l_pos, rev.l_pos[::-1]) and np.array_equal(fwd.l_neg, rev.l_neg[::-1])
        one = windows.score_windows([seq], pos, neg, window=window, step=step, method='likelihood')
        assert not np.array_equal(one.scores, fwd.scores)


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------
def test_end_to_end_one_insert_is_one_region(tmp_path):
    """200 kb from the order-3 chain of negative row 2000 with 30 kb of positive row 2200's at base 100 000, both rows taken
    out of the reference, 500-base blocks.  Seed and rows were fixed after statement (i) alone, on CPU-computed likelihood
    scores, recovered the insert exactly (blocks 200..259) where the threshold called 15 regions; seed 3 does the same
    (11 regions)."""
    from phamers_amd import fileIO, segment, windows
    g = helpers.load_npz("ref_features.npz")
    pos, neg = g["pos_counts"].astype(np.int64), g["neg_counts"].astype(np.int64)
    seq = ref.chain_sequence(np.random.default_rng(2), [neg[2000], pos[2200], neg[2000]], [0, 100000, 130000, 200000], 200000)
    rp, rn = np.delete(pos, 2200, axis=0), np.delete(neg, 2000, axis=0)
    fasta, out = str(tmp_path / "genome.fasta"), str(tmp_path / "out")
    with open(fasta, "w") as f:
        f.write(">genome\n" + "\n".join(seq[i:i + 80] for i in range(0, len(seq), 80)) + "\n")
    fileIO.save_counts(rp, ["p%d" % i for i in range(len(rp))], str(tmp_path / "pos.csv"))
    fileIO.save_counts(rn, ["n%d" % i for i in range(len(rn))], str(tmp_path / "neg.csv"))
    track, regions = windows.main(["-in", fasta, "-out", out, "-pf", str(tmp_path / "pos.csv"), "-nf", str(tmp_path / "neg.csv"),
                                   "-m", "likelihood", "-w", "500", "-s", "500", "--segment"])
    assert len(track) == 400 and np.isfinite(track.scores).all()
    seg = segment.segment_track(track)
    trans, init, qt, qp = quantised(seg.p_enter, seg.p_leave)
    states, score = ref.viterbi(ref.quantise(track.scores), qt, qp)   # (i) on the device's own scores; temper is 1
    assert seg.temper == 1.0 and np.array_equal(seg.state, states) and int(seg.path_score[0] * 2 ** 16) == score
    found = seg.regions()
    assert len(found) == 1
    rid, start, end, n_windows = found[0][:4]
    assert rid == "genome" and abs(start - 100000) <= 1000 and abs(end - 130000) <= 1000 and n_windows == (end - start) // 500
    assert len(regions) > 1 and regions == windows.call_regions(track)     # the bare threshold splits it
    assert segment.read_segments(out + "/phage_segments.csv") == found
    ref.check(seg.posterior, seg.log_odds[0], seg.x, trans, init, what="end to end")
