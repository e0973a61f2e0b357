"""GPU: the boundary refinement (phamers_amd/csrc/refine.hip) against its statement in Python ints
(tests/refine_ref.py): every output ``array_equal``.  k = 4 (the difference row in LDS), k = 6 (both rows from global memory)
and k = 1; in one call intervals that are empty, lie inside one packed word, start and end at every offset of a word, cover
1023 / 1024 / 1025 / 2049 k-mer starts (the pass boundary and the carry), reach a sequence's last base, sit at the stream's
pad word and in a sequence of fewer than k bases; x at lo, at hi and between; invalid bases singly, over a whole interval and
across a lane's and a pass's edge; the ties; all d < 0 and all d > 0; a table of +-2^31; equal rows; more boundaries than one
pass of the grid; the boundaries shuffled and each alone; the ASCII and the FASTA entry; the errors; and
``segment_sequences(refine=True)`` end to end."""
import numpy as np
import pytest

from tests import compose_ref as cref
from tests import refine_ref as rref

pytestmark = pytest.mark.gpu
WORDS_BEFORE = 7            # the main sequence starts 7 * 16 + 5 bases into the stream: at offset 5 of a packed word
MAIN = 1                    # its index


def device(seqs, k, q, bounds, symbols=b"ATGC", source=None):
    from phamers_amd import _lib
    cols = [np.array([b[i] for b in bounds], dtype=np.int64) for i in range(6)]
    pos, ev, sup = _lib.refine_boundaries(_lib.get_context(), seqs if source is None else source, k, symbols, q, *cols)
    return pos, ev, sup.astype(np.int64)


def statement(seqs, k, q, bounds):
    cols = [[b[i] for b in bounds] for i in range(6)]
    return rref.refine(seqs, k, q, *cols)


def assert_same(got, want, what=""):
    for name, g, w in zip(("position", "evidence", "support"), got, want):
        assert np.array_equal(g, w), (what, name, np.flatnonzero((np.asarray(g) != np.asarray(w)).reshape(len(w), -1).any(axis=1))[:8])


def make_case(k):
    """(sequences, table, boundaries (seq, lo, x, hi, left_row, right_row)) of the call of many shapes."""
    from phamers_amd import segment
    rng = np.random.default_rng(40 + k)
    D = 4 ** k
    q = segment.quantise(np.log(rng.dirichlet(np.full(D, 0.7), 3)))
    first = "".join("ATGC"[d] for d in rng.integers(0, 4, 16 * WORDS_BEFORE + 5))
    L = 7000
    main = ["ATGC"[d] for d in rng.integers(0, 4, L)]
    base = len(first)                                     # stream position of the main sequence's base 0
    at = lambda stream: stream - base                     # sequence position of a stream position
    word = lambda w, o=0: at(16 * (w + WORDS_BEFORE + 1) + o)   # offset o of the w-th whole word of the main sequence
    # invalid bases: singly; across a lane's edge (the last base of a word and the first of the next); a run over a whole
    # interval; across a pass's edge (1024 starts after the word in which an interval below begins)
    for p in (word(3, 7), word(40, 0), word(41, 15), word(52, 15), word(53, 0)):
        main[p] = "N"
    for p in range(word(60, 2), word(63, 9)):
        main[p] = "N"
    for p in (word(100 + 64, -2), word(100 + 64, -1), word(100 + 64, 0), word(100 + 64, 1)):
        main[p] = "n"
    main = "".join(main)
    short = "ACGTAC"[:k - 1]
    last = "".join("ATGC"[d] for d in rng.integers(0, 4, 333))
    seqs = [first, main, short, "", last]
    bounds, rows = [], [(0, 1), (1, 2), (2, 0), (1, 0)]

    def add(seq, lo, hi, where, r=None):
        x = lo if where == 0 else hi if where == 1 else (lo + hi) // 2 if where == 2 else lo + (hi - lo) // 3
        left, right = rows[len(bounds) % 4] if r is None else r
        bounds.append((seq, lo, x, hi, left, right))
    add(MAIN, 100, 100, 0)                                                 # empty
    add(MAIN, 0, 0, 0)
    add(MAIN, L, L, 0)
    add(MAIN, word(2, 3), word(2, 9), 2)                                   # inside one word
    add(MAIN, word(3, 5), word(3, 10), 1)                                  # ... holding an invalid base
    for a in range(16):                                                    # every start and end offset of a word
        for e in range(16):
            add(MAIN, word(10 + a, a), word(13 + a, e), (a + e) % 4)
    for n in (1023, 1024, 1025, 2049):                                     # the pass boundary and the carry
        for o in (0, 5, 15):
            add(MAIN, word(100, o), word(100, o) + n, (n + o) % 4)
            add(MAIN, word(230, o), word(230, o) + n, (n + o + 1) % 4)
    add(MAIN, L - 40, L, 2)                                                # the sequence's last base: k - 1 invalid starts
    add(MAIN, L - 3, L, 0)
    add(MAIN, L - 2100, L, 3)
    add(4, len(last) - 50, len(last), 2)                                   # the last sequence, at the stream's pad word
    add(4, 0, len(last), 1)
    add(4, len(last) - 1, len(last), 1)
    add(2, 0, len(short), 2)                                               # fewer than k bases
    add(2, 0, 0, 0)
    add(3, 0, 0, 0)                                                        # no base at all
    add(0, 0, len(first), 2)                                               # up to the next sequence: no k-mer runs into it
    add(0, len(first) - k, len(first), 0)
    add(MAIN, word(60, 2), word(63, 9), 2)                                 # invalid bases over the whole interval
    add(MAIN, word(60, 4), word(63, 5), 3)
    add(MAIN, word(59, 0), word(64, 0), 2)                                 # ... and with valid ones on either side
    add(MAIN, word(52, 3), word(53, 12), 2)                                # across a lane's edge
    add(MAIN, word(40, 0), word(42, 0), 1)
    for r in ((0, 0), (2, 2)):                                             # equal rows: all zeros, position x
        add(MAIN, word(20, 3), word(90, 1), 3, r)
    return seqs, q, bounds


@pytest.fixture(scope="module")
def cases():
    out = {}
    for k in (4, 6, 1):
        seqs, q, bounds = make_case(k)
        out[k] = (seqs, q, bounds, statement(seqs, k, q, bounds))
    return out


@pytest.mark.parametrize("k", [4, 6, 1])
def test_one_call_of_many_shapes(cases, k):
    seqs, q, bounds, want = cases[k]
    got = device(seqs, k, q, bounds)
    assert_same(got, want, "k = %d" % k)
    pos, ev, sup = want
    assert (ev >= 0).all()
    lo, x, hi = (np.array([b[i] for b in bounds]) for i in (1, 2, 3))
    assert ((lo <= pos) & (pos <= hi)).all()
    none = sup == 0                                                        # without evidence a boundary stays at x
    assert none.sum() >= 8 and np.array_equal(pos[none], x[none]) and not ev[none].any()
    equal = np.array([b[4] == b[5] for b in bounds])
    assert equal.sum() == 2 and np.array_equal(pos[equal], x[equal]) and not ev[equal].any() and (sup[equal] > 0).all()
    assert (pos != x).sum() > len(bounds) // 2                             # (the case does move boundaries)


@pytest.mark.parametrize("k", [4, 6, 1])
def test_locality_shuffled_and_alone(cases, k):
    seqs, q, bounds, want = cases[k]
    order = np.random.default_rng(9).permutation(len(bounds))
    got = device(seqs, k, q, [bounds[i] for i in order])
    assert_same(got, [w[order] for w in want], "shuffled, k = %d" % k)
    # each alone (at k = 4 every boundary, else every fifth) with its sequence the only one of the call: another place in the
    # stream, another offset in the packed words
    for i in range(0, len(bounds), 1 if k == 4 else 5):
        b = bounds[i]
        alone = device([seqs[b[0]]], k, q, [(0,) + b[1:]])
        assert_same(alone, [w[i:i + 1] for w in want], "boundary %d alone, k = %d" % (i, k))


def test_more_boundaries_than_one_pass_of_the_grid(cases):
    from phamers_amd import _lib
    seqs, q, _, _ = cases[4]
    n = _lib.refine_grid_pass() + 3
    assert n == 8195
    L = len(seqs[MAIN])
    bounds = []
    for i in range(n):
        lo = (7919 * i) % (L - 20)
        hi = lo + 3 + i % 14
        bounds.append((MAIN, lo, lo + i % (hi - lo + 1), hi, i % 3, (i + 1 + i % 2) % 3))
    assert_same(device(seqs, 4, q, bounds), statement(seqs, 4, q, bounds), "grid pass + 3")


def tie_table():
    """k = 1: d(A) = +1, d(T) = -1, d(G) = d(C) = 0 between rows 0 and 1; rows 2 and 3: all d > 0 / all d < 0 against row 1."""
    return np.array([[1, -1, 0, 0], [0, 0, 0, 0], [3, 1, 2, 5], [-3, -1, -2, -5]], dtype=np.int64)


def test_ties_and_signs():
    q = tie_table()
    flat = "G" * 3000
    peaks = lambda gap: "A" + "T" + "G" * gap + "A" + "T"                   # P = 1 at p = 1 and at p = gap + 3, else 0
    seqs = [flat, peaks(2), peaks(40), peaks(1100), "ATGC" * 600]
    bounds = []
    for lo, x, hi in ((0, 1500, 3000), (7, 7, 2100), (7, 2100, 2100), (100, 101, 130), (0, 0, 3000)):
        bounds.append((0, lo, x, hi, 0, 1))                                # flat on both sides of x: position x
    for s, gap in ((1, 2), (2, 40), (3, 1100)):                            # the maxima in one lane, two lanes, two passes
        n = gap + 4
        mid = (1 + gap + 3) // 2                                           # gap even: both maxima at the same distance
        for x in (mid, mid - 1, mid + 1, 0, 1, n, gap + 3):
            bounds.append((s, 0, x, n, 0, 1))
    for lo, hi in ((0, 2400), (3, 1030), (17, 18), (5, 2054)):
        for x in (lo, hi, (lo + hi) // 2):
            bounds.append((4, lo, x, hi, 2, 1))                            # all d > 0: position hi
            bounds.append((4, lo, x, hi, 3, 1))                            # all d < 0: position lo
            bounds.append((4, lo, x, hi, 1, 2))
    want = statement(seqs, 1, q, bounds)
    assert_same(device(seqs, 1, q, bounds), want, "ties")
    pos = want[0]
    assert pos[:5].tolist() == [1500, 7, 2100, 101, 0]
    for j, gap in enumerate((2, 40, 1100)):                                # equal distance: the smaller position; else the nearer
        assert pos[5 + 7 * j:12 + 7 * j].tolist() == [1, 1, gap + 3, 1, 1, gap + 3, gap + 3], gap
    signs = np.array(bounds[26:])
    assert np.array_equal(pos[26::3], signs[0::3, 3]) and np.array_equal(pos[27::3], signs[1::3, 1])
    assert np.array_equal(pos[28::3], signs[2::3, 1])


@pytest.mark.parametrize("k", [4, 6])
def test_extreme_table_needs_64_bits(k):
    """2049 starts of one k-mer at d = +-2^32: a 32-bit or a float accumulator would fail."""
    D = 4 ** k
    q = np.zeros((3, D), dtype=np.int64)
    q[0], q[1] = 2 ** 31, -2 ** 31
    q[2, 0], q[2, 1:] = -2 ** 31, 2 ** 31 - 1                              # AAAA.. low, every other k-mer high
    seqs = ["A" * (2049 + k - 1), "A" * 1000 + "ATGCATGGC" + "A" * 1200]
    bounds = [(0, 0, 1000, 2049, 0, 1), (0, 0, 1000, 2049, 1, 0), (0, 0, 0, 2049, 0, 2), (0, 5, 2049, 2049, 2, 0),
              (1, 0, 1100, 2209, 0, 1), (1, 3, 900, 2100, 2, 0), (1, 3, 900, 2100, 0, 2)]
    want = statement(seqs, k, q, bounds)
    assert_same(device(seqs, k, q, bounds), want, "extreme")
    assert want[1][0].tolist() == [1049 * 2 ** 32, 2049 * 2 ** 32, 0] and want[0][:2].tolist() == [2049, 0]
    assert want[2][0] == 2049


def test_ascii_and_fasta_entries(cases, tmp_path):
    from phamers_amd import _lib, refine, segment
    seqs, q, bounds, want = cases[4]
    path = str(tmp_path / "in.fasta")
    with open(path, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">s%d\n" % i + "".join(s[j:j + 70] + "\n" for j in range(0, len(s), 70)))
    fasta = _lib.Fasta(path)
    try:
        assert fasta.lengths().tolist() == [len(s) for s in seqs]
        assert_same(device(None, 4, q, bounds, source=fasta), want, "fasta")
    finally:
        fasta.close()
    assert_same(device(seqs, 4, q, bounds), want, "ascii")
    # the Python entry: profiles in, quantised by segment.quantise; a path or the strings
    logp = np.log(np.random.default_rng(3).dirichlet(np.full(256, 0.7), 3))
    cols = [np.array([b[i] for b in bounds]) for i in range(6)]
    spos, sev, ssup = rref.refine(seqs, 4, segment.quantise(logp), *cols)
    for source in (path, seqs):
        r = refine.boundaries(source, 4, logp, *cols)
        assert np.array_equal(r.position, spos) and np.array_equal(r.support, ssup)
        assert np.array_equal(np.stack([r.gain, r.left_evidence, r.right_evidence], axis=1), sev)
        assert np.array_equal(r.gain_nats, sev[:, 0] * 2.0 ** -16)
    # another alphabet: the columns follow the symbols' order
    rna = [s.replace("T", "U") for s in seqs]
    assert_same(device(rna, 4, q, bounds, symbols=b"AUGC"), want, "AUGC")
    swapped = rref.refine(seqs, 4, q, *[[b[i] for b in bounds] for i in range(6)], symbols="CGTA")
    assert_same(device(seqs, 4, q, bounds, symbols=b"CGTA"), swapped, "CGTA")


def test_errors(cases):
    from phamers_amd import _lib
    seqs, q, bounds, _ = cases[4]
    L = len(seqs[MAIN])
    good = (MAIN, 10, 20, 30, 0, 1)
    assert_same(device(seqs, 4, q, [good]), statement(seqs, 4, q, [good]))
    for bad in ((5, 10, 20, 30, 0, 1),                                     # no such sequence
                (MAIN, 10, 20, 30, 3, 1), (MAIN, 10, 20, 30, 0, 3),        # no such row
                (MAIN, 21, 20, 30, 0, 1), (MAIN, 10, 31, 30, 0, 1),        # lo > x, x > hi
                (MAIN, 10, 20, L + 1, 0, 1), (2, 0, 0, 4, 0, 1),           # hi > L
                (MAIN, 0, 5, 2 ** 30 + 1, 0, 1)):                          # more than 2^30 bases
        with pytest.raises(ValueError):
            device(seqs, 4, q, [good, bad])
    with pytest.raises(ValueError, match="2\\^30"):
        device(seqs, 4, q, [(MAIN, 0, 5, 2 ** 30 + 1, 0, 1)])
    with pytest.raises(ValueError):
        device(seqs, 3, q, [good])                                         # D is not 4^k
    with pytest.raises(ValueError):
        device(seqs, 0, q[:, :1], [good])
    with pytest.raises(_lib.PhkError):
        device(seqs, 8, np.zeros((1, 4 ** 8), dtype=np.int64), [good])     # k above the library's
    for v in (2 ** 31 + 1, -2 ** 31 - 1):
        big = q.copy()
        big[2, 255] = v
        with pytest.raises(ValueError):
            device(seqs, 4, big, [good])
    edge = q.copy()
    edge[2, 255], edge[1, 0] = 2 ** 31, -2 ** 31                           # the limits themselves are taken
    assert_same(device(seqs, 4, edge, [good]), statement(seqs, 4, edge, [good]))
    with pytest.raises(ValueError):
        device(seqs, 4, q, [good], symbols=b"ATG")
    # B = 0: nothing to do, with no array at all; a NULL where B > 0 is refused
    ctx = _lib.get_context()
    bases = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    offsets = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.uint64)
    qq = np.ascontiguousarray(q)
    call = lambda B, position: ctx.lib.phk_refine_boundaries_ascii(
        ctx.handle, _lib.ptr(bases), _lib.ptr(offsets), len(seqs), 4, b"ATGC", _lib.ptr(qq), 3, 256, *(cols + [B, position, out_e, out_s]))
    cols, out_e, out_s = [None] * 6, None, None
    assert call(0, None) == _lib.PHK_OK
    one = [np.array([v], dtype=np.uint64) for v in good[:4]] + [np.array([v], dtype=np.uint32) for v in good[4:]]
    pos, ev, sup = np.zeros(1, dtype=np.int64), np.zeros((1, 3), dtype=np.int64), np.zeros(1, dtype=np.uint32)
    cols, out_e, out_s = [_lib.ptr(a) for a in one], _lib.ptr(ev), _lib.ptr(sup)
    assert call(1, None) == _lib.PHK_ERR_ARG
    assert call(1, _lib.ptr(pos)) == _lib.PHK_OK
    assert (int(pos[0]), ev[0].tolist(), int(sup[0])) == (lambda w: (int(w[0][0]), w[1][0].tolist(), int(w[2][0])))(statement(seqs, 4, q, [good]))
    cols[2] = None
    assert call(1, _lib.ptr(pos)) == _lib.PHK_ERR_ARG


# ---- end to end -------------------------------------------------------------------------------------------------------------
E2E_SEED, E2E_BOUNDS = 3, [0, 13230, 26770, 40000]
# Chosen on the CPU with the statement in the place of the device (the fit by tests/compose_ref.py's E-step): seeds 1 .. 8 of
# this sequence give refined positions 1 to 132 bases from the true change points, the window boundaries 230 to 270; seed 3
# gives the positions 13235 and 26771 -- 5 and 1 bases off -- where the window grid says 13000 and 27000, 230 off each.
E2E_STATEMENT_POSITIONS, E2E_WINDOW_BOUNDARIES = [13235, 26771], [13000, 27000]


def test_end_to_end_segment_sequences():
    from phamers_amd import compose, segment
    from tests import segment_ref
    rows = cref.small_rows()
    seq = segment_ref.chain_sequence(np.random.default_rng(E2E_SEED), [rows[0], rows[1], rows[0]], E2E_BOUNDS, E2E_BOUNDS[-1])
    result = compose.segment_sequences([seq], 2, refine=True)
    plain = compose.segment_sequences([seq], 2)
    assert plain.boundaries is None and np.array_equal(plain.state, result.state) and plain.regions() == result.regions()
    # the statement applied to the device's decode and the device's profiles
    rec, x, lo, hi, ls, rs, _ = rref.boundary_plan(result.state, result.owner, result.start, 500, 500)
    pos, ev, sup = rref.refine([seq], 4, segment.quantise(result.composition.log_profiles), rec, lo, x, hi, ls, rs)
    b = result.boundaries
    assert np.array_equal(b.position, pos) and np.array_equal(b.evidence_q, ev) and np.array_equal(b.support, sup)
    assert np.array_equal(b.window_boundary, x) and b.record_id == ["0"] * len(pos)
    regions, fine = result.regions(), result.refined_regions()
    assert len(fine) == len(regions) == len(pos) + 1
    want = [list(r) for r in regions]
    for j, p in enumerate(pos):
        want[j][2] = want[j + 1][1] = int(p)
    assert fine == [tuple(r) for r in want]
    assert fine[0][1] == 0 and fine[-1][2] == 40000
    # every refined position is nearer the true change point than the window boundary
    true = E2E_BOUNDS[1:-1]
    assert len(pos) == len(true)
    d_fine, d_grid = [abs(int(p) - t) for p, t in zip(pos, true)], [abs(int(v) - t) for v, t in zip(x, true)]
    print("refined", pos.tolist(), d_fine, "grid", list(x), d_grid, "gain (nats)", b.gain.tolist())
    assert all(f < g for f, g in zip(d_fine, d_grid)), (d_fine, d_grid)
    assert (b.gain > 0).all()
