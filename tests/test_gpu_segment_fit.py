"""GPU: the E-step and the Baum-Welch loop of the segmentation chain (csrc/segment.hip, phamers_amd/segment.py
``expected_counts`` / ``fit``) against the statements of tests/segment_fit_ref.py: a record's
expected counts within the derived bound (v) of the longdouble statement (i) and of the brute force (ii), consistent with the
existing decode within the sum of the two bounds, bit for bit the same whatever else the call holds; the totals bit for bit
the tree (iv) of the device's own per-record values; every M-step bit for bit statement (iii).  T = PHK_SEG_TILE = 64."""
import numpy as np
import pytest

from tests import helpers, segment_fit_ref as fref, segment_ref as ref

pytestmark = pytest.mark.gpu

T = 64
A, B = 0.05, 0.1
LENGTHS = [1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, 64 * T + 1]
LD = ref.LD


def owners(n):
    return np.zeros(n, dtype=np.int64) if n else [0, 0]


def counts_of(e):
    """(R, 6) as the library lays a record's counts out."""
    return np.concatenate((e.transitions, e.start), axis=1)


def check_invariants(e, d, x, off, what=""):
    """A call's expected counts ``e`` against the decode ``d`` of the same call: the sums of the pairwise posteriors over
    the state left are the sums of the decode's posteriors, within the sum of the two bounds; log_odds bit for bit."""
    assert np.array_equal(e.log_odds, d.log_odds), what
    for r in range(len(off) - 1):
        lo, hi = int(off[r]), int(off[r + 1])
        n = hi - lo
        xi, g0 = e.transitions[r].astype(LD), e.start[r].astype(LD)
        if n == 0:
            assert not xi.any() and not g0.any(), (what, r)
            continue
        post = d.posterior[lo:hi].astype(LD)
        Bp, Bx = ref.posterior_bound(n), fref.xi_bound(n)
        into1, into0 = post[1:].sum(), (LD(1) - post[1:]).sum()
        assert abs((xi[1] + xi[3]) - into1) <= (Bp + Bx + 2 * ref.U) * into1 + 2 * n * ref.FLOOR, (what, r, xi, into1)
        assert abs((xi[0] + xi[2]) - into0) <= (n - 1) * Bp + (Bx + 2 * ref.U) * into0 + 2 * n * ref.FLOOR, (what, r, xi, into0)
        assert abs(xi.sum() - (n - 1)) <= (Bx + 4 * ref.U) * (n - 1), (what, r, xi)
        assert abs(g0[1] - post[0]) <= 2 * Bp * post[0] + 2 * ref.FLOOR, (what, r, g0, post[0])
        assert abs(g0.sum() - 1) <= 2 * Bp, (what, r, g0)


# ---- 1. single records -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_one_record_against_the_statement_and_the_decode(n):
    from phamers_amd import segment
    x = ref.biased_evidence(np.random.default_rng(100 + n), n)
    for kw in (dict(), dict(p_start=0.5, temper=0.25)):
        e = segment.expected_counts(x, owners(n), A, B, **kw)
        assert e.transitions.shape == (1, 4) and e.start.shape == (1, 2) and e.log_odds.shape == (1,) and e.totals.shape == (6,)
        assert e.transitions.dtype == e.start.dtype == e.totals.dtype == np.float64
        trans, init = ref.parameters(A, B, kw.get("p_start"))
        xs = kw.get("temper", 1.0) * x
        fref.check_record(counts_of(e)[0], e.log_odds[0], xs, trans, init, what="n=%d %r" % (n, kw))
        assert np.array_equal(e.totals, counts_of(e)[0]) and e.log_evidence == e.log_odds[0]      # one record: no addition
        if n == 1:
            assert not e.transitions.any()
        check_invariants(e, segment.decode(x, owners(n), A, B, **kw), xs, [0, n], what="n=%d" % n)


@pytest.mark.parametrize("a,b,s", [(0.05, 0.1, None), (0.5, 0.5, 0.5), (1e-3, 0.3, 0.9)])
def test_short_records_against_the_brute_force(a, b, s):
    from phamers_amd import segment
    rng = np.random.default_rng(int(1000 * a))
    trans, init = ref.parameters(a, b, s)
    for n in (1, 2, 3, 7, 12):
        for case in range(3):
            x = ref.biased_evidence(rng, n, run=3)
            if case == 1:
                x = np.rint(x) * (rng.random(n) < 0.6)       # exact ties and zeros
            if case == 2:
                x[:] = 0.0
            e = segment.expected_counts(x, owners(n), a, b, p_start=s)
            xi, g0, lo = fref.brute_force(x, trans, init)
            fref.check_record(counts_of(e)[0], e.log_odds[0], x, trans, init, what="brute n=%d" % n, want=(xi, g0, lo))


# ---- 2. ragged calls ---------------------------------------------------------------------------------------------------------
def ragged_case(records=300, seed=7):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 5 * T + 1, records)
    lengths[[0, 10, 11, records - 1]] = 0            # empty records first, adjacent and last
    lengths[[1, 2, 3, 4]] = [T, 5 * T, 1, T + 1]
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    return ref.biased_evidence(rng, int(off[-1])), off


def test_ragged_records_equal_each_record_alone_in_any_order_and_run():
    from phamers_amd import segment
    x, off = ragged_case()
    R = len(off) - 1
    e = segment.expected_counts(x, off, A, B)
    again = segment.expected_counts(x, off, A, B)
    assert all(np.array_equal(u, v) for u, v in zip(e, again))                         # run to run
    check_invariants(e, segment.decode(x, off, A, B), x, off, what="ragged")
    trans, init = ref.parameters(A, B)
    for r in (1, 2, 3, 4, 150):
        fref.check_record(counts_of(e)[r], e.log_odds[r], x[int(off[r]):int(off[r + 1])], trans, init, what="ragged %d" % r)
    for r in range(R):
        lo, hi = int(off[r]), int(off[r + 1])
        one = segment.expected_counts(x[lo:hi], owners(hi - lo), A, B)
        assert np.array_equal(counts_of(one)[0], counts_of(e)[r]) and one.log_odds[0] == e.log_odds[r], r
        if hi == lo:
            assert not counts_of(e)[r].any() and e.log_odds[r] == 0.0
        if hi - lo == 1:
            assert not e.transitions[r].any() and e.start[r].sum() > 0.5
    # the totals are the tree of the device's own per-record values, bit for bit
    assert np.array_equal(e.totals, fref.tree_sum(counts_of(e)))
    assert e.log_evidence == fref.tree_sum(e.log_odds[:, None])[0]
    # the records in reversed order
    pieces = [x[int(off[r]):int(off[r + 1])] for r in range(R)][::-1]
    roff = np.concatenate(([0], np.cumsum([len(p) for p in pieces]))).astype(np.uint64)
    rev = segment.expected_counts(np.concatenate(pieces), roff, A, B)
    assert np.array_equal(counts_of(rev), counts_of(e)[::-1]) and np.array_equal(rev.log_odds, e.log_odds[::-1])
    assert np.array_equal(rev.totals, fref.tree_sum(counts_of(rev)))


def test_more_tiles_than_one_grid_pass():
    """70 000 records of 1..3 windows are more tiles than one launch covers, and more than 256 blocks of the reduction:
    the same records in calls that stay below the pass, a sample of records alone, and the tree over all of them."""
    from phamers_amd import _lib, segment
    grid_pass = int(_lib.load().phk_segment_grid_pass())
    rng = np.random.default_rng(11)
    R = 70000
    assert R > grid_pass + 64 and -(-R // 256) > 256
    lengths = rng.integers(1, 4, R)
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    x = ref.biased_evidence(rng, int(off[-1]))
    e = segment.expected_counts(x, off, A, B)
    c = counts_of(e)
    assert np.isfinite(c).all() and (c >= 0).all() and np.isfinite(e.log_odds).all()
    assert np.array_equal(e.totals, fref.tree_sum(c)) and e.log_evidence == fref.tree_sum(e.log_odds[:, None])[0]
    assert fref.tree_levels(R) == 3
    assert abs(e.totals[:4].sum() - (int(off[-1]) - R)) <= 1e-9 * int(off[-1]) and abs(e.totals[4:].sum() - R) <= 1e-9 * R
    cuts = np.linspace(0, R, 5).astype(int)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        a, b = int(off[lo]), int(off[hi])
        part = segment.expected_counts(x[a:b], off[lo:hi + 1] - off[lo], A, B)
        assert np.array_equal(counts_of(part), c[lo:hi]) and np.array_equal(part.log_odds, e.log_odds[lo:hi])
    trans, init = ref.parameters(A, B)
    for r in sorted(set(rng.integers(0, R, 16).tolist()) | set(range(R - 8, R))):
        lo, hi = int(off[r]), int(off[r + 1])
        one = segment.expected_counts(x[lo:hi], owners(hi - lo), A, B)
        assert np.array_equal(counts_of(one)[0], c[r]) and one.log_odds[0] == e.log_odds[r], r
        fref.check_record(c[r], e.log_odds[r], x[lo:hi], trans, init, what="record %d" % r)


# ---- 3. extremes -------------------------------------------------------------------------------------------------------------
def extreme_cases(n=3 * T + 5):
    rng = np.random.default_rng(5)
    flip = np.repeat(rng.choice([-1.0, 1.0], n // 9 + 1), 9)[:n]
    return {"zero": np.zeros(n), "+800": np.full(n, 800.0), "-800": np.full(n, -800.0), "+-800": 800.0 * flip,
            "+-2^16": 2.0 ** 16 * flip}


@pytest.mark.parametrize("b", [1e-12, 0.5, 1 - 1e-12])
@pytest.mark.parametrize("a", [1e-12, 0.5, 1 - 1e-12])
def test_extreme_evidence_and_parameters(a, b):
    from phamers_amd import segment
    for name, x in extreme_cases().items():
        n = len(x)
        e = segment.expected_counts(x, owners(n), a, b)
        c = counts_of(e)
        assert np.isfinite(c).all() and (c >= 0).all() and np.isfinite(e.log_odds).all(), (name, c)
        check_invariants(e, segment.decode(x, owners(n), a, b), x, [0, n], what="%s a=%g b=%g" % (name, a, b))


# ---- 4. error codes ----------------------------------------------------------------------------------------------------------
def test_errors_before_any_launch():
    from phamers_amd import _lib, segment
    ctx = _lib.get_context()
    x = np.ones(5)
    trans, init = ref.parameters(A, B)

    def rc(x=x, off=(0, 5), trans=trans, init=init):
        off = np.asarray(off, dtype=np.uint64)
        R = len(off) - 1
        out = np.empty((R, 6)), np.empty(6), np.empty(R), np.empty(1)
        return ctx.lib.phk_segment_expect(ctx.handle, _lib.ptr(np.ascontiguousarray(x, dtype=np.float64)), len(x), _lib.ptr(off), R,
                                          _lib.ptr(np.ascontiguousarray(trans)), _lib.ptr(np.ascontiguousarray(init)),
                                          *[_lib.ptr(o) for o in out])
    assert rc() == _lib.PHK_OK
    for bad in ([0.0, 1.0, B, 1 - B], [1 - A, A, 1.0, 0.0], [1 - A, A + 1e-9, B, 1 - B], [np.nan, A, B, 1 - B]):
        assert rc(trans=np.array(bad)) == _lib.PHK_ERR_ARG, bad
    for bad in ([0.0, 1.0], [0.5, 0.5 + 1e-9], [np.nan, 0.5]):
        assert rc(init=np.array(bad)) == _lib.PHK_ERR_ARG, bad
    for bad in ((1, 5), (0, 4), (0, 6), (0, 3, 2, 5)):
        assert rc(off=bad) == _lib.PHK_ERR_ARG, bad
    assert rc(x=np.array([1.0, np.inf, 1.0, 1.0, 1.0])) == _lib.PHK_ERR_NAN
    assert rc(x=np.zeros(0), off=(0,)) == _lib.PHK_OK and rc(x=np.zeros(0), off=(0, 0, 0)) == _lib.PHK_OK
    # the counts and log_odds may be NULL; the totals are the same
    tot, ev = np.empty(6), np.empty(1)
    off = np.array([0, 2, 5], dtype=np.uint64)
    assert ctx.lib.phk_segment_expect(ctx.handle, _lib.ptr(x), 5, _lib.ptr(off), 2, _lib.ptr(trans), _lib.ptr(init), None,
                                      _lib.ptr(tot), None, _lib.ptr(ev)) == _lib.PHK_OK
    e = segment.expected_counts(x, off, A, B)
    assert np.array_equal(tot, e.totals) and ev[0] == e.log_evidence
    empty = segment.expected_counts(np.zeros(0), [0, 0, 0], A, B)
    assert empty.transitions.shape == (2, 4) and not counts_of(empty).any() and not empty.totals.any()
    assert empty.log_evidence == 0.0 and np.array_equal(empty.log_odds, [0.0, 0.0])
    none = segment.fit(np.zeros(0), [0, 0, 0], A, B)
    assert none.n_iter == 1 and none.converged and none.no_transitions and (none.p_enter, none.p_leave) == (A, B)
    with pytest.raises(ValueError):
        segment.fit([1.0, np.inf], [0, 2], A, B)
    for kw in (dict(start=[0.0, B, 0.5]), dict(start=[A, 1.0, 0.5]), dict(start=[A, B, 0.0], start_mode=0),
               dict(start_mode=3), dict(prior_counts=[0, 0, -1.0, 0]), dict(tol=-1.0), dict(tol=np.nan)):
        args = dict(start=[A, B, 0.5], start_mode=2, prior_counts=[0.0] * 4, max_iter=3, tol=1e-8)
        args.update(kw)
        with pytest.raises(ValueError):
            _lib.segment_fit(ctx, x, [0, 5], **args)
    assert _lib.segment_fit(ctx, x, [0, 5], [A, B, 0.0], 2, [0.0] * 4, 3, 1e-8)[1] >= 1   # stationary: start[2] is not read


# ---- 5. the fit --------------------------------------------------------------------------------------------------------------
MODES = {"fixed": fref.FIXED, "free": fref.FREE, "stationary": fref.STATIONARY}


def check_trace(f, x, mode, prior=(0.0, 0.0, 0.0, 0.0), what=""):
    """Every row's totals and evidence against statement (i) AT the row's parameters, every next row's parameters bit for
    bit statement (iii) of the row's totals; the evidence monotone up to the bound for the exact modes."""
    status, bounds = 0, []
    for i, row in enumerate(f.trace):
        a, b, s = row[:3]
        trans, init = ref.parameters(a, b, s)
        bounds.append(fref.check_totals(row[3:9], row[9], x, trans, init, what="%s row %d" % (what, i))[2])
        if i + 1 < len(f.trace):
            params, bits = fref.m_step(row[3:9], (a, b, s), prior, MODES[mode])
            assert params == tuple(f.trace[i + 1, :3]), (what, i, params, f.trace[i + 1, :3])
            status |= bits
    L = f.trace[:, 9]
    if mode != "stationary" and not any(prior):
        for i in range(1, len(L)):
            assert L[i] - L[i - 1] >= -(bounds[i] + bounds[i - 1]), (what, i, L)
    assert L[-1] == L.max() and f.log_evidence == L[-1]
    assert tuple(f.trace[-1, :3]) == (f.p_enter, f.p_leave, f.p_start)
    return status


@pytest.fixture(scope="module")
def small_tracks():
    return fref.sample_chain(np.random.default_rng(21), 8, 200, 0.02, 0.1)[0]


@pytest.mark.parametrize("mode", ["fixed", "free", "stationary"])
def test_fit_iterations_against_the_statements(small_tracks, mode):
    from phamers_amd import segment
    x = small_tracks
    off = np.arange(0, x.size + 1, x.shape[1]).astype(np.uint64)
    p_start = 0.3 if mode == "fixed" else mode
    f = segment.fit(x.ravel(), off, 0.1, 0.3, p_start=p_start, max_iter=40, tol=1e-9)
    assert f.converged and 2 <= f.n_iter <= 40 and f.trace.shape == (f.n_iter + 1, 10) and not f.no_transitions
    assert f.trace[0, 0] == 0.1 and f.trace[0, 1] == 0.3 and f.trace[0, 2] == (0.3 if mode == "fixed" else 0.1 / (0.1 + 0.3))
    check_trace(f, x, mode, what=mode)
    if mode == "fixed":
        assert (f.trace[:, 2] == 0.3).all()
    assert f.log_evidence > f.trace[0, 9]
    # row 0 is expected_counts at the start parameters, bit for bit; max_iter cuts the same trace short
    e = segment.expected_counts(x.ravel(), off, 0.1, 0.3, p_start=f.trace[0, 2])
    assert np.array_equal(f.trace[0, 3:9], e.totals) and f.trace[0, 9] == e.log_evidence
    g = segment.fit(x.ravel(), off, 0.1, 0.3, p_start=p_start, max_iter=2, tol=0.0)
    assert g.n_iter == 2 and not g.converged and np.array_equal(g.trace, f.trace[:3])
    # prior counts enter the M-step as stated
    h = segment.fit(x.ravel(), off, 0.1, 0.3, p_start=p_start, prior_counts=(5.0, 1.0, 2.0, 7.0), max_iter=3, tol=0.0)
    assert h.n_iter >= 1
    check_trace(h, x, mode, prior=(5.0, 1.0, 2.0, 7.0), what=mode + " with prior")
    assert not np.array_equal(h.trace[1, :2], f.trace[1, :2])


def test_fit_status_bits():
    from phamers_amd import segment
    # an all-negative track: nothing ever enters the phage state, p_enter runs into its clamp
    x = np.full(400, -30.0)
    off = np.arange(0, 401, 100).astype(np.uint64)
    f = segment.fit(x, off, 0.05, 0.1, p_start=0.01, max_iter=20)
    assert f.clamped and f.p_enter == 1e-12 and f.converged
    check_trace(f, x.reshape(4, 100), "fixed", what="all negative")
    # records of one window have no transition: both rows keep their parameters, and the evidence cannot move
    x = ref.biased_evidence(np.random.default_rng(4), 10)
    f = segment.fit(x, np.arange(11).astype(np.uint64), 0.05, 0.1, p_start=0.3)
    assert f.no_transitions and f.converged and not f.clamped and f.n_iter == 1
    assert (f.p_enter, f.p_leave, f.p_start) == (0.05, 0.1, 0.3) and not f.trace[:, 3:7].any()
    assert f.trace[0, 9] == f.trace[1, 9] and abs(f.trace[0, 7:9].sum() - 10) < 1e-12
    free = segment.fit(x, np.arange(11).astype(np.uint64), 0.05, 0.1, p_start='free')
    assert free.no_transitions and (free.p_enter, free.p_leave) == (0.05, 0.1) and free.log_evidence >= free.trace[0, 9]
    check_trace(free, x.reshape(10, 1), "free", what="one window")


def test_fit_recovers_the_chain_the_tracks_were_drawn_from():
    """The recovery data of tests/test_segment_fit_host.py: 64 records of 1 500 windows from (0.004, 0.04), started at
    ``segment_track``'s defaults at step 500."""
    from phamers_amd import segment
    x, _ = fref.sample_chain(np.random.default_rng(7), 64, 1500, 0.004, 0.04)
    b0 = 500.0 / 30000.0
    a0 = b0 * 0.05 / (1.0 - 0.05)
    off = np.arange(0, x.size + 1, 1500).astype(np.uint64)
    f = segment.fit(x.ravel(), off, a0, b0, max_iter=50, tol=1e-6)
    assert f.converged and not f.clamped and not f.no_transitions
    assert abs(f.p_enter - 0.004) <= 0.2 * 0.004 and abs(f.p_leave - 0.04) <= 0.2 * 0.04, (f.p_enter, f.p_leave)
    check_trace(f, x, "stationary", what="recovery")


def test_segment_track_with_fit_is_fit_track_then_the_decode():
    from phamers_amd import segment, windows
    x, _ = fref.sample_chain(np.random.default_rng(9), 3, 300, 0.02, 0.08)
    scores = np.concatenate((x[0], x[1][:170], x[2]))
    scores[40:44] = np.nan                                                # no evidence: the chain carries
    owner = np.repeat([0, 2, 3], [300, 170, 300])                         # record 1 has no window
    start = np.concatenate([np.arange(k) * 500 for k in (300, 170, 300)])
    track = windows.WindowTrack(["a", "b", "c", "d"], owner, start, 500, 500, scores)
    f = segment.fit_track(track, mean_region=10000, phage_fraction=0.1, max_iter=30)
    assert f.converged and f.n_iter >= 2 and f.mean_region == 500.0 / f.p_leave
    assert f.phage_fraction == f.p_enter / (f.p_enter + f.p_leave) and f.temper == 1.0
    seg = segment.segment_track(track, mean_region=10000, phage_fraction=0.1, fit=True, max_iter=30)
    assert np.array_equal(seg.fit.trace, f.trace) and (seg.p_enter, seg.p_leave) == (f.p_enter, f.p_leave)
    d = segment.decode(track.scores, track.owner, f.p_enter, f.p_leave, f.p_start, temper=f.temper)
    assert np.array_equal(seg.posterior, d.posterior) and np.array_equal(seg.state, d.state)
    assert np.array_equal(seg.log_odds[[0, 2, 3]], d.log_odds[[0, 2, 3]]) and np.array_equal(seg.path_score, d.path_score)
    assert f.log_evidence == fref.tree_sum(seg.log_odds[:, None])[0]     # the last row is the returned chain's evidence
    plain = segment.segment_track(track, mean_region=10000, phage_fraction=0.1)
    assert plain.fit is None and plain.p_leave == 0.05 and plain.log_odds.sum() < seg.log_odds.sum()


# ---- 6. the command line -----------------------------------------------------------------------------------------------------
def test_command_line_fit_on_the_sequence_with_one_insert(tmp_path):
    """The 200 kb sequence with a 30 kb insert of tests/test_gpu_segment.py, ``--segment --fit``.  The number of regions
    under the fitted chain is deliberately not asserted (profiles/segment_fit/README.md records it)."""
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
    track, _ = windows.main(["-in", fasta, "-out", out, "-pf", str(tmp_path / "pos.csv"), "-nf", str(tmp_path / "neg.csv"),
                             "-m", "likelihood", "-w", "500", "-s", "500", "--segment", "--fit"])
    rows = segment.read_fit(out + "/segment_fit.csv")
    evidence = [r[6] for r in rows]
    assert len(rows) >= 2 and [r[0] for r in rows] == list(range(len(rows)))
    assert all(after >= before for before, after in zip(evidence[:-1], evidence[1:])), evidence
    unfitted = segment.segment_track(track)
    assert rows[0][1:3] == (unfitted.p_enter, unfitted.p_leave) and evidence[0] == unfitted.log_odds[0]
    assert evidence[-1] >= unfitted.log_odds[0]
    fitted = segment.segment_track(track, fit=True)
    assert rows[-1][1:4] == (fitted.p_enter, fitted.p_leave, fitted.fit.p_start) and evidence[-1] == fitted.log_odds[0]
    assert segment.read_segments(out + "/phage_segments.csv") == fitted.regions()
    print("regions under the fitted chain: %d, fit rows: %r" % (len(fitted.regions()), rows))
