"""GPU: the boundary confidence (phamers_amd/csrc/refine.hip) against its statement
(tests/refine_confidence_ref.py) on the call of many shapes of tests/test_gpu_refine.py -- k = 4 (the difference row in LDS),
k = 6 (both rows from global memory) and k = 1; empty intervals, every word offset, 1023 / 1024 / 1025 / 2049 starts, invalid
runs, sequence ends, the pad word.  position, evidence and support ``array_equal`` to ``phk_refine_boundaries_*`` on the same
call; the interval ``array_equal`` to the statement at drop_q = 0, 1, 3 * 2^16 and 2^62 (every candidate); the five sums
within the derived bound; the inequalities.  Then: a table of +-2^31 (most weights past the 700-nat cut), equal rows, all d < 0
and all d > 0, a tie class split in two by a dip, more boundaries than one pass of the grid, the boundaries shuffled and each
alone (the sums ``array_equal``), the ASCII and the FASTA entry, the Python entries, the refusals, and the behavioural case."""
import numpy as np
import pytest

from tests import refine_confidence_ref as fref
from tests.test_gpu_refine import MAIN, make_case, tie_table

pytestmark = pytest.mark.gpu
DROPS = (0, 1, 3 << 16, 1 << 62)


def columns(bounds):
    return [np.array([b[i] for b in bounds], dtype=np.int64) for i in range(6)]


def device(seqs, k, q, bounds, drop_q, symbols=b"ATGC", source=None):
    from phamers_amd import _lib
    pos, ev, sup, interval, sums = _lib.refine_confidence(_lib.get_context(), seqs if source is None else source, k, symbols, q,
                                                          *columns(bounds), drop_q)
    assert interval.dtype == np.int64 and interval.shape == (len(bounds), 3) and sums.dtype == np.float64 and sums.shape == (len(bounds), 5)
    return pos, ev, sup.astype(np.int64), interval, sums


def plain(seqs, k, q, bounds, symbols=b"ATGC", source=None):
    from phamers_amd import _lib
    pos, ev, sup = _lib.refine_boundaries(_lib.get_context(), seqs if source is None else source, k, symbols, q, *columns(bounds))
    return pos, ev, sup.astype(np.int64)


def statement(seqs, k, q, bounds, symbols="ATGC"):
    return fref.Statement(seqs, k, q, *[[b[i] for b in bounds] for i in range(6)], symbols=symbols)


def check(seqs, k, q, bounds, drops=DROPS, what="", st=None):
    """One device call per drop against the old entry and the statement; the statement and the last call's outputs."""
    st = statement(seqs, k, q, bounds) if st is None else st
    old = plain(seqs, k, q, bounds)
    lo, hi = np.array(st.lo), np.array(st.hi)
    first = None
    for drop_q in drops:
        got = device(seqs, k, q, bounds, drop_q)
        for name, g, o, w in zip(("position", "evidence", "support"), got, old, (st.position, st.evidence, st.support)):
            assert np.array_equal(g, o) and np.array_equal(g, w), (what, drop_q, name)
        pos, interval, sums = got[0], got[3], got[4]
        want = st.interval(drop_q)
        assert np.array_equal(interval, want), (what, drop_q, np.flatnonzero((interval != want).any(axis=1))[:8])
        worst = fref.assert_sums_within(sums, st.sums(drop_q), st.n, (what, drop_q))
        print("%s drop_q = %d: worst error of a sum = %.3f of its bound" % (what, drop_q, worst))
        lower, upper, n_within = interval.T
        assert ((lo <= lower) & (lower <= pos) & (pos <= upper) & (upper <= hi)).all()
        assert ((1 <= n_within) & (n_within <= upper - lower + 1)).all() and (sums[:, 0] >= 1).all() and (sums >= 0).all()
        assert (sums[:, 1] <= sums[:, 0]).all()
        if first is None:
            first = sums
        for c in (0, 2, 3, 4):                                             # Z, S1_left, S1_right and S2 do not see the drop
            assert np.array_equal(sums[:, c], first[:, c]), (what, drop_q, c)
        if drop_q == 1 << 62:                                              # every candidate
            assert np.array_equal(n_within, st.n) and np.array_equal(lower, lo) and np.array_equal(upper, hi)
            assert np.array_equal(sums[:, 1], sums[:, 0])
    return st, got


@pytest.fixture(scope="module")
def cases():
    out = {}
    for k in (4, 6, 1):
        seqs, q, bounds = make_case(k)
        out[k] = (seqs, q, bounds, statement(seqs, k, q, bounds))
    return out


@pytest.mark.parametrize("k", [4, 6, 1])
def test_one_call_of_many_shapes(cases, k):
    seqs, q, bounds, st = cases[k]
    _, got = check(seqs, k, q, bounds, what="k = %d" % k, st=st)
    empty = st.n == 1
    assert empty.sum() >= 5
    assert np.array_equal(got[3][empty], np.stack([st.lo, st.lo, np.ones(len(st.lo), dtype=np.int64)], axis=1)[empty])
    assert np.array_equal(got[4][empty], np.tile([1.0, 1.0, 0.0, 0.0, 0.0], (int(empty.sum()), 1)))
    equal = np.array([b[4] == b[5] for b in bounds])                       # equal rows: all P = 0, every weight 1
    assert equal.sum() == 2
    n = st.n[equal].astype(np.float64)
    assert np.array_equal(st.interval(0)[equal][:, 2], st.n[equal]) and np.array_equal(got[4][equal][:, 0], n)
    at3 = st.interval(3 << 16)
    assert (at3[:, 2] < st.n).sum() > len(bounds) // 2                     # (the drop does leave candidates out)


@pytest.mark.parametrize("k", [4, 6, 1])
def test_locality_shuffled_and_alone(cases, k):
    """The eight numbers of a boundary are the same bits in another order, and alone with its sequence the only one of the
    call: another place in the stream, another offset in the packed words."""
    seqs, q, bounds, st = cases[k]
    drop_q = 3 << 16
    whole = device(seqs, k, q, bounds, drop_q)
    order = np.random.default_rng(9).permutation(len(bounds))
    got = device(seqs, k, q, [bounds[i] for i in order], drop_q)
    for name, g, w in zip(("position", "evidence", "support", "interval", "sums"), got, whole):
        assert np.array_equal(g, w[order]), ("shuffled", k, name)
    for i in range(0, len(bounds), 2 if k == 4 else 5):
        b = bounds[i]
        alone = device([seqs[b[0]]], k, q, [(0,) + b[1:]], drop_q)
        for name, g, w in zip(("position", "evidence", "support", "interval", "sums"), alone, whole):
            assert np.array_equal(g, w[i:i + 1]), ("boundary %d alone" % i, k, name, g, w[i:i + 1])


def test_more_boundaries_than_one_pass_of_the_grid(cases):
    from phamers_amd import _lib
    seqs, q, _, _ = cases[4]
    n = _lib.refine_grid_pass() + 3
    L = len(seqs[MAIN])
    bounds = []
    for i in range(n):
        lo = (7919 * i) % (L - 20)
        hi = lo + 3 + i % 14
        bounds.append((MAIN, lo, lo + i % (hi - lo + 1), hi, i % 3, (i + 1 + i % 2) % 3))
    check(seqs, 4, q, bounds, drops=(1 << 15, 1 << 62), what="grid pass + 3")


@pytest.mark.parametrize("k", [4, 6])
def test_extreme_table_most_weights_past_the_cut(k):
    """2049 starts at d = +-2^32 (65536 nats a base): one candidate at the maximum, every other weight exactly 0."""
    D = 4 ** k
    q = np.zeros((3, D), dtype=np.int64)
    q[0], q[1] = 2 ** 31, -2 ** 31
    q[2, 0], q[2, 1:] = -2 ** 31, 2 ** 31 - 1
    seqs = ["A" * (2049 + k - 1), "A" * 1000 + "ATGCATGGC" + "A" * 1200]
    bounds = [(0, 0, 1000, 2049, 0, 1), (0, 0, 1000, 2049, 1, 0), (0, 0, 0, 2049, 0, 2), (0, 5, 2049, 2049, 2, 0),
              (1, 0, 1100, 2209, 0, 1), (1, 3, 900, 2100, 2, 0), (1, 3, 900, 2100, 0, 2)]
    st, got = check(seqs, k, q, bounds, what="extreme, k = %d" % k)
    assert st.position[:2].tolist() == [2049, 0] and st.evidence[0].tolist() == [1049 * 2 ** 32, 2049 * 2 ** 32, 0]
    assert got[4][:2].tolist() == [[1, 1, 0, 0, 0]] * 2                    # (2^62 selects all 2050: M = Z = 1 all the same)
    assert st.interval(3 << 16)[:2].tolist() == [[2049, 2049, 1], [0, 0, 1]]


def test_signs_and_the_ends():
    """All d > 0: the maximum at hi, ``upper`` = hi; all d < 0: at lo; in units of a quarter nat, so that weights count."""
    from phamers_amd import refine
    q = tie_table() << 14
    seqs = ["ATGC" * 600]
    bounds = []
    for lo, hi in ((0, 2400), (3, 1030), (17, 18), (5, 2054)):
        for x in (lo, hi, (lo + hi) // 2):
            bounds.append((0, lo, x, hi, 2, 1))                            # all d > 0
            bounds.append((0, lo, x, hi, 3, 1))                            # all d < 0
    st, got = check(seqs, 1, q, bounds, what="signs")
    hi, lo = np.array(st.hi), np.array(st.lo)
    iv = st.interval(3 << 16)
    assert np.array_equal(st.position[0::2], hi[0::2]) and np.array_equal(st.position[1::2], lo[1::2])
    assert np.array_equal(iv[0::2, 1], hi[0::2]) and np.array_equal(iv[1::2, 0], lo[1::2])
    c = refine.confidence_from_sums(lo, hi, iv, got[4])
    assert c.at_hi[0::2].all() and c.at_lo[1::2].all()
    wide = st.n > 40
    assert not c.at_lo[0::2][wide[0::2]].any() and not c.at_hi[1::2][wide[1::2]].any()
    assert (c.mean_offset[0::2][wide[0::2]] < 0).all() and (c.mean_offset[1::2][wide[1::2]] > 0).all()


def test_a_tie_class_split_by_a_dip():
    """P = one nat at p = 1 and at p = gap + 3, 0 between and after: at a drop below the dip the set is two points, the range
    between them is not in it, and M counts the dip's weights all the same.  The maxima in one lane, two lanes, two passes."""
    one = 1 << 16
    q = tie_table() * one
    peaks = lambda gap: "A" + "T" + "G" * gap + "A" + "T"
    seqs = [peaks(2), peaks(40), peaks(1100)]
    bounds = [(s, 0, x, gap + 4, 0, 1) for s, gap in enumerate((2, 40, 1100)) for x in (0, (gap + 4) // 2, gap + 4)]
    st, got = check(seqs, 1, q, bounds, drops=(0, one - 1, one, 1 << 62), what="dip")
    gaps = np.repeat([2, 40, 1100], 3)
    e = np.exp(-1.0)
    for drop_q in (0, one - 1):
        interval, sums = device(seqs, 1, q, bounds, drop_q)[3:]
        assert np.array_equal(interval, np.stack([np.ones(9, dtype=np.int64), gaps + 3, np.full(9, 2)], axis=1))
        assert (interval[:, 2] < interval[:, 1] - interval[:, 0] + 1).all()
        assert np.allclose(sums[:, 1], 2 + (gaps + 1) * e, rtol=1e-12, atol=0) and np.allclose(sums[:, 0], 2 + (gaps + 3) * e, rtol=1e-12, atol=0)
    interval = device(seqs, 1, q, bounds, one)[3]
    assert np.array_equal(interval, np.stack([np.zeros(9, dtype=np.int64), gaps + 4, gaps + 5], axis=1))


def test_ascii_and_fasta_entries_and_the_python_entry(cases, tmp_path):
    from phamers_amd import _lib, refine, segment
    seqs, q, bounds, st = cases[4]
    path = str(tmp_path / "in.fasta")
    with open(path, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">s%d\n" % i + "".join(s[j:j + 70] + "\n" for j in range(0, len(s), 70)))
    drop_q = 3 << 16
    whole = device(seqs, 4, q, bounds, drop_q)
    fasta = _lib.Fasta(path)
    try:
        got = device(None, 4, q, bounds, drop_q, source=fasta)
        old = plain(None, 4, q, bounds, source=fasta)
    finally:
        fasta.close()
    for name, g, w in zip(("position", "evidence", "support", "interval", "sums"), got, whole):
        assert np.array_equal(g, w), name
    for g, o in zip(got, old):
        assert np.array_equal(g, o)
    # the Python entry: profiles in, a drop in nats; a path or the strings; beside refine.boundaries
    logp = np.log(np.random.default_rng(3).dirichlet(np.full(256, 0.7), 3))
    cols = columns(bounds)
    want = fref.Statement(seqs, 4, segment.quantise(logp), *cols)
    before = refine.boundaries(seqs, 4, logp, *cols)
    results = [refine.confidence(source, 4, logp, *cols, drop=1.25) for source in (path, seqs)]
    for r, c in results:
        for name, g, w in zip(r._fields, r, before):
            assert np.array_equal(g, w), name
        assert np.array_equal(np.stack([c.lower, c.upper, c.n_within], axis=1), want.interval(5 << 14))
        assert np.array_equal(c.at_lo, c.lower == cols[1]) and np.array_equal(c.at_hi, c.upper == cols[3])
        fref.assert_sums_within(c.sums, want.sums(5 << 14), want.n, "python entry")
        fref.assert_derived_within(c, want.sums(5 << 14), want.n, "python entry")
        assert np.array_equal(c.sums, results[0][1].sums)
    # another alphabet
    rna = [s.replace("T", "U") for s in seqs]
    for g, w in zip(device(rna, 4, q, bounds, drop_q, symbols=b"AUGC"), whole):
        assert np.array_equal(g, w)


def test_errors(cases):
    from phamers_amd import _lib
    seqs, q, bounds, _ = cases[4]
    L = len(seqs[MAIN])
    good = (MAIN, 10, 20, 30, 0, 1)
    check(seqs, 4, q, [good], drops=(0, 7), what="good")
    for drop_q in (-1, -2 ** 63):
        with pytest.raises(ValueError, match="drop_q"):
            device(seqs, 4, q, [good], drop_q)
    with pytest.raises(ValueError):
        device(seqs, 4, q, [good], 2 ** 63)
    device(seqs, 4, q, [good], 2 ** 63 - 1)                                # the largest int64 is taken
    for bad in ((5, 10, 20, 30, 0, 1), (MAIN, 10, 20, 30, 3, 1), (MAIN, 10, 20, 30, 0, 3), (MAIN, 21, 20, 30, 0, 1),
                (MAIN, 10, 31, 30, 0, 1), (MAIN, 10, 20, L + 1, 0, 1), (2, 0, 0, 4, 0, 1), (MAIN, 0, 5, 2 ** 30 + 1, 0, 1)):
        with pytest.raises(ValueError):
            device(seqs, 4, q, [good, bad], 5)
    with pytest.raises(ValueError):
        device(seqs, 3, q, [good], 5)                                      # D is not 4^k
    with pytest.raises(_lib.PhkError):
        device(seqs, 8, np.zeros((1, 4 ** 8), dtype=np.int64), [good], 5)  # k above the library's
    big = q.copy()
    big[2, 255] = 2 ** 31 + 1
    with pytest.raises(ValueError):
        device(seqs, 4, big, [good], 5)
    with pytest.raises(ValueError):
        device(seqs, 4, q, [good], 5, symbols=b"ATG")
    # B = 0: nothing to do, with no array at all (a negative drop is refused all the same); a NULL where B > 0 is refused
    ctx = _lib.get_context()
    bases = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    offsets = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.uint64)
    qq = np.ascontiguousarray(q)
    call = lambda B, drop_q, outs: ctx.lib.phk_refine_confidence_ascii(
        ctx.handle, _lib.ptr(bases), _lib.ptr(offsets), len(seqs), 4, b"ATGC", _lib.ptr(qq), 3, 256, *(cols + [B, drop_q] + outs))
    cols = [None] * 6
    assert call(0, 0, [None] * 5) == _lib.PHK_OK and call(0, -1, [None] * 5) == _lib.PHK_ERR_ARG
    one = [np.array([v], dtype=np.uint64) for v in good[:4]] + [np.array([v], dtype=np.uint32) for v in good[4:]]
    arrays = [np.zeros(1, dtype=np.int64), np.zeros((1, 3), dtype=np.int64), np.zeros(1, dtype=np.uint32),
              np.zeros((1, 3), dtype=np.int64), np.zeros((1, 5), dtype=np.float64)]
    cols = [_lib.ptr(a) for a in one]
    outs = [_lib.ptr(a) for a in arrays]
    for missing in range(5):
        assert call(1, 0, outs[:missing] + [None] + outs[missing + 1:]) == _lib.PHK_ERR_ARG, missing
    assert call(1, 0, outs) == _lib.PHK_OK
    st = statement(seqs, 4, q, [good])
    assert int(arrays[0][0]) == st.position[0] and np.array_equal(arrays[3], st.interval(0))
    fref.assert_sums_within(arrays[4], st.sums(0), st.n)


def test_the_join_lies_in_the_interval_and_a_close_pair_is_wider():
    """The behavioural case of tests/test_refine_confidence_host.py on the device: first device == statement, then the join
    inside [lower, upper] at 3 nats for every listed seed, and the close pair's median width above the far pair's."""
    from phamers_amd import refine, segment
    widths = {}
    for kind in ("far", "close"):
        cases = [fref.behaviour_case(kind, seed) for seed in fref.BEHAVIOUR_SEEDS]
        widths[kind] = []
        for seq, logp in cases:
            cols = ([0], [fref.BEHAVIOUR_LO], [fref.BEHAVIOUR_X], [fref.BEHAVIOUR_HI], [0], [1])
            r, c = refine.confidence([seq], 4, logp, *cols, drop=3.0)
            st = fref.Statement([seq], 4, segment.quantise(logp), *cols)
            assert np.array_equal(r.position, st.position) and np.array_equal(r.left_evidence, st.evidence[:, 1])
            assert np.array_equal(np.stack([c.lower, c.upper, c.n_within], axis=1), st.interval(3 << 16))
            fref.assert_sums_within(c.sums, st.sums(3 << 16), st.n, kind)
            fref.assert_derived_within(c, st.sums(3 << 16), st.n, kind)
            assert c.lower[0] <= fref.BEHAVIOUR_JOIN <= c.upper[0], (kind, c.lower, c.upper)
            widths[kind].append(int(c.upper[0] - c.lower[0]))
    print("widths", widths)
    assert widths == fref.BEHAVIOUR_STATEMENT_WIDTHS
    assert np.median(widths["close"]) > np.median(widths["far"])


def test_segment_sequences_with_confidence():
    """End to end on the sequence of tests/test_gpu_refine.py: the boundaries are those of the call without, the confidence
    the statement's on the device's decode and profiles."""
    from phamers_amd import compose, segment
    from tests import compose_ref as cref
    from tests import refine_ref as rref
    from tests import segment_ref
    from tests.test_gpu_refine import E2E_BOUNDS, E2E_SEED
    rows = cref.small_rows()
    seq = segment_ref.chain_sequence(np.random.default_rng(E2E_SEED), [rows[0], rows[1], rows[0]], E2E_BOUNDS, E2E_BOUNDS[-1])
    without = compose.segment_sequences([seq], 2, refine=True)
    result = compose.segment_sequences([seq], 2, refine=True, confidence=True)
    assert without.boundary_confidence is None
    for name, g, w in zip(result.boundaries._fields, result.boundaries, without.boundaries):
        assert (g == w) if isinstance(g, list) else np.array_equal(g, w), name
    assert result.refined_regions() == without.refined_regions()
    rec, x, lo, hi, ls, rs, _ = rref.boundary_plan(result.state, result.owner, result.start, 500, 500)
    st = fref.Statement([seq], 4, segment.quantise(result.composition.log_profiles), rec, lo, x, hi, ls, rs)
    c = result.boundary_confidence
    assert len(c.lower) == 2 and np.array_equal(np.stack([c.lower, c.upper, c.n_within], axis=1), st.interval(3 << 16))
    fref.assert_sums_within(c.sums, st.sums(3 << 16), st.n, "end to end")
    print("intervals", c.lower.tolist(), result.boundaries.position.tolist(), c.upper.tolist(), "true", E2E_BOUNDS[1:-1],
          "mass within", c.mass_within.tolist())
    with pytest.raises(ValueError):
        compose.segment_sequences([seq], 2, confidence=True)
