"""GPU: grouped chains (chain.hip) -- every group of a grouped call against a fresh chain on that
group's records alone, bit for bit (emissions, expectations, decode; from host rows, a resident batch and two batch_rows),
the Viterbi path against the integer recurrence and the float results against the bounds of tests/compose_ref.py, the
active mask, the order of the groups, more groups than one launch covers, the mode's errors, and ``compose.fit_groups``
against ``compose.fit`` per scaffold.  Shapes: the records of tests/test_gpu_compose.py and one more, cut into a one-window
group, a group without records, a group holding an empty record, two-record groups and a last group of 1090 windows that
crosses a reduction block and starts at a window that is no multiple of 128; S = 2 .. 8 at D = 256, S = 3 and 8 at D = 30;
more groups than one launch at every padded width (S = 2, 4, 5).  Fold levels past the first, the tables of one chain under
changing masks and more than one column group are tests/test_gpu_chain_shapes.py's."""
import csv
import os

import numpy as np
import pytest

from tests import compose_groups_ref as gref
from tests import compose_ref as cref
from tests.test_gpu_compose import chain_parameters, make_case, run

pytestmark = pytest.mark.gpu
LD = cref.LD
LENGTHS = [1, 2, 63, 0, 64, 65, 129, 1, 1000, 90]
GROUPS = np.array([0, 1, 1, 4, 5, 7, 8, 10], dtype=np.uint64)
KEYS = [(2, 256), (3, 256), (4, 256), (5, 256), (6, 256), (7, 256), (8, 256), (3, 30), (8, 30)]
OUTPUTS = ("E", "T", "Ns", "xi", "gamma0", "L", "L_rec", "state", "posterior", "le", "score")


def group_case(S, D, lengths=LENGTHS, groups=GROUPS):
    """The rows of ``make_case`` with parameters of its own for every group."""
    c = make_case(S, D, lengths=lengths)
    rng = np.random.default_rng(77 * S + D)
    G = len(groups) - 1
    logp = np.array([np.log((lambda p: p / p.sum(axis=1, keepdims=True))(np.exp(c["logp"] + 0.2 * rng.standard_normal((S, D)))))
                     for _ in range(G)])
    par = [chain_parameters(rng, S, 0.6 + 0.35 * rng.random()) for _ in range(G)]
    return dict(c, groups=np.asarray(groups, dtype=np.uint64), glogp=logp, gpar=par)


def stacked(case):
    par = case["gpar"]
    return [np.array([p[i] for p in par]) for i in range(4)]


def run_grouped(case, batch_rows=0, resident=False, active=None):
    from phamers_amd import _lib
    ctx = _lib.get_context()
    batch = _lib.Batch.from_counts(ctx, case["counts"]) if resident else None
    assert not resident or batch is not None
    chain = _lib.Chain(ctx, batch if resident else case["counts"], case["offsets"], case["S"], batch_rows)
    try:
        chain.set_groups(case["groups"])
        A, pi, qt, qp = stacked(case)
        chain.set_grouped(case["glogp"], A, pi, qt, qp, case["temper"], active)
        out = dict(E=chain.emissions())
        out["T"], out["Ns"], out["xi"], out["gamma0"], out["L"], out["L_rec"] = chain.expect_grouped(records=True)
        out["state"], out["posterior"], out["le"], out["score"] = chain.decode()
    finally:
        chain.close()
        if batch is not None:
            batch.close()
    return out


def alone(case, g):
    """A fresh chain on group g's records alone, with ``set`` and g's parameters."""
    rows, off = gref.group_rows(case["counts"], case["offsets"], case["groups"], g)
    return run(dict(case, counts=np.ascontiguousarray(rows), offsets=off, logp=case["glogp"][g], par=case["gpar"][g]))


def group_part(case, out, g):
    """Group g's part of a grouped result, shaped as ``alone`` returns it."""
    r0, r1, w0, w1 = gref.group_spans(case["offsets"], case["groups"])[g]
    return dict(E=out["E"][w0:w1], T=out["T"][g], Ns=out["Ns"][g], xi=out["xi"][g], gamma0=out["gamma0"][g], L=out["L"][g],
                L_rec=out["L_rec"][r0:r1], state=out["state"][w0:w1], posterior=out["posterior"][w0:w1], le=out["le"][r0:r1],
                score=out["score"][r0:r1])


def differing(a, b):
    return [k for k in OUTPUTS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for S, D in KEYS:
        c = group_case(S, D)
        c["got"] = run_grouped(c)
        c["alone"] = [alone(c, g) for g in range(len(GROUPS) - 1)]
        out[(S, D)] = c
    return out


@pytest.mark.parametrize("key", KEYS)
def test_every_group_equals_the_group_alone(cases, key):
    c = cases[key]
    spans = gref.group_spans(c["offsets"], c["groups"])
    assert [s[3] - s[2] for s in spans] == [1, 0, 65, 64, 194, 1, 1090] and spans[6][2] % 128 != 0
    for kw in (dict(), dict(resident=True), dict(batch_rows=1), dict(batch_rows=1025), dict(resident=True, batch_rows=1025)):
        if kw.get("resident") and key[1] != 256:
            continue                                                   # (a resident batch has 4^k columns)
        got = c["got"] if not kw else run_grouped(c, **kw)
        for g in range(len(spans)):
            assert differing(group_part(c, got, g), c["alone"][g]) == [], (kw, g)
    assert not c["got"]["T"][1].any() and c["got"]["L"][1] == 0.0        # the group without records: zeros


@pytest.mark.parametrize("key", KEYS)
def test_viterbi_and_the_bounds_of_the_statement_per_group(cases, key):
    c, got = cases[key], cases[key]["got"]
    S = c["S"]
    for g in range(len(GROUPS) - 1):
        rows, off = gref.group_rows(c["counts"], c["offsets"], c["groups"], g)
        part = group_part(c, got, g)
        A, pi, qt, qp = c["gpar"][g]
        off = off.astype(int)
        n, R = len(rows), len(off) - 1
        states, scores = cref.viterbi_records(part["E"], off, qt, qp)
        assert np.array_equal(part["state"], states) and part["score"].tolist() == scores, g
        if n == 0:
            continue
        exact = cref.exact_emissions(rows, c["glogp"][g], c["temper"])
        assert (np.abs(part["E"].astype(LD) - exact).astype(np.float64) <= cref.emission_bound(rows, c["glogp"][g], c["temper"])).all()
        longest = int(np.diff(off).max())
        want = cref.expect(part["E"], off, A, pi, rows)
        cref.check_posterior(part["posterior"], want["gamma"], longest, S, "posterior of group %d" % g)
        M = part["E"].max(axis=1)
        total = LD(0)
        for r in range(R):
            b = cref.evidence_bound(M[off[r]:off[r + 1]], S, want["log_evidence_rec"][r])
            assert abs(LD(part["le"][r]) - want["log_evidence_rec"][r]) <= b, (g, r)
            total += b
        assert np.array_equal(part["le"], part["L_rec"])
        total += R * cref.U * float(np.abs(want["log_evidence_rec"]).sum())
        assert abs(LD(part["L"]) - want["log_evidence"]) <= total, g
        cref.check_sums(part["xi"], want["xi"], longest, S, n + R, n, "xi")
        cref.check_sums(part["gamma0"], want["gamma0"], longest, S, R, R, "gamma0")
        cref.check_sums(part["T"], want["T"], longest, S, n, float(rows.sum()), "T")
        cref.check_sums(part["Ns"], want["Ns"], longest, S, n, n, "Ns")


@pytest.mark.parametrize("key", [(3, 256), (8, 30)])
def test_inactive_groups_are_passed_over(cases, key):
    from phamers_amd import _lib
    c = cases[key]
    G = len(GROUPS) - 1
    active = np.ones(G, dtype=bool)
    active[[2, 6]] = False
    garbage = dict(c, glogp=c["glogp"].copy(), gpar=[tuple(np.array(x) for x in p) for p in c["gpar"]])
    for g in (2, 6):                                                   # not read: NaN is no error there
        garbage["glogp"][g] = np.nan
        garbage["gpar"][g] = (np.full((c["S"], c["S"]), np.nan), np.full(c["S"], np.nan)) + garbage["gpar"][g][2:]
    for case in (c, garbage):
        got = run_grouped(case, active=active)
        for g in range(G):
            part = group_part(c, got, g)
            if active[g]:
                assert differing(part, c["alone"][g]) == [], g
            else:
                assert all(not np.asarray(part[k]).any() for k in OUTPUTS), g
    # the same garbage in an active group is refused before any launch, and the next call is clean
    ctx = _lib.get_context()
    chain = _lib.Chain(ctx, c["counts"], c["offsets"], c["S"])
    try:
        chain.set_groups(c["groups"])
        A, pi, qt, qp = stacked(c)
        gA, gpi, _, _ = stacked(garbage)
        with pytest.raises(ValueError):
            chain.set_grouped(garbage["glogp"], A, pi, qt, qp, c["temper"])              # PHK_ERR_NAN
        with pytest.raises(ValueError):
            chain.set_grouped(c["glogp"], gA, pi, qt, qp, c["temper"])                   # PHK_ERR_ARG
        with pytest.raises(ValueError):
            chain.set_grouped(c["glogp"], A, gpi, qt, qp, c["temper"])
        with pytest.raises(ValueError):
            chain.set_grouped(c["glogp"], A, pi, -qt - 1, qp, c["temper"])
        with pytest.raises(ValueError):
            chain.set_grouped(c["glogp"], A, pi, qt, qp, 0.0)
        with pytest.raises(ValueError):
            chain.expect_grouped()                                     # the failed sets left no parameters behind
        chain.set_grouped(c["glogp"], A, pi, qt, qp, c["temper"])
        T, Ns, xi, g0, L = chain.expect_grouped()
    finally:
        chain.close()
    assert np.array_equal(T, c["got"]["T"]) and np.array_equal(xi, c["got"]["xi"]) and np.array_equal(L, c["got"]["L"])


@pytest.mark.parametrize("key", [(3, 256), (5, 256), (8, 30)])
def test_the_order_of_the_groups_does_not_matter(cases, key):
    c = cases[key]
    G = len(GROUPS) - 1
    spans = gref.group_spans(c["offsets"], c["groups"])
    lengths = np.diff(c["offsets"].astype(np.int64))
    for order in (np.random.default_rng(key[0]).permutation(G), np.arange(G)[::-1]):
        rows = np.concatenate([np.arange(spans[g][2], spans[g][3]) for g in order]).astype(int)
        rec = np.concatenate([lengths[spans[g][0]:spans[g][1]] for g in order])
        moved = dict(c, counts=np.ascontiguousarray(c["counts"][rows]),
                     offsets=np.concatenate(([0], np.cumsum(rec))).astype(np.uint64),
                     groups=np.concatenate(([0], np.cumsum([spans[g][1] - spans[g][0] for g in order]))).astype(np.uint64),
                     glogp=c["glogp"][order], gpar=[c["gpar"][g] for g in order])
        got = run_grouped(moved)
        for i, g in enumerate(order):
            assert differing(group_part(moved, got, i), c["alone"][g]) == [], (order.tolist(), g)


@pytest.mark.parametrize("S", [2, 4, 5])
def test_more_groups_than_one_launch_covers(S):
    from phamers_amd import _lib
    D, pad = 30, 2 if S <= 2 else (4 if S <= 4 else 8)
    G = int(_lib.load().phk_chain_grid_pass()) + 300
    edge = int(_lib.load().phk_chain_grid_pass()) * 2 // pad           # the first record past one launch at this width
    base = group_case(S, D, lengths=[2] * 7, groups=np.arange(8))
    which = np.arange(G) % 7
    rows = (2 * which[:, None] + np.arange(2)[None, :]).reshape(-1)
    case = dict(base, counts=np.ascontiguousarray(base["counts"][rows]), offsets=(2 * np.arange(G + 1)).astype(np.uint64),
                groups=np.arange(G + 1, dtype=np.uint64), glogp=base["glogp"][which], gpar=[base["gpar"][g] for g in which])
    got = run_grouped(case)
    for k in ("T", "Ns", "xi", "gamma0", "L", "L_rec", "le", "score"):
        assert np.array_equal(got[k], got[k][:7][which]), k
    for k in ("E", "state", "posterior"):
        per = got[k].reshape((G, 2) + got[k].shape[1:])
        assert np.array_equal(per, per[:7][which]), k
    for g in list(range(7)) + [G - 1, edge]:
        assert differing(group_part(case, got, g), alone(case, g)) == [], g


def test_the_errors_of_the_mode(cases):
    from phamers_amd import _lib
    ctx = _lib.get_context()
    c = cases[(3, 256)]
    A, pi, qt, qp = stacked(c)
    one = c["gpar"][0]
    chain = _lib.Chain(ctx, c["counts"], c["offsets"], 3)
    try:
        with pytest.raises(ValueError):
            chain.set_grouped(c["glogp"], A, pi, qt, qp, c["temper"])    # grouped calls on a chain without groups
        with pytest.raises(ValueError):
            chain.expect_grouped()
        for bad in ([0, 1, 1, 5, 4, 7, 8, 10], [0, 4, 9], [1, 10], [0, 4, 11]):
            with pytest.raises(ValueError):
                chain.set_groups(bad)
        chain.set(c["logp"], *one, c["temper"])
        plain = chain.expect(records=True), chain.decode()
        chain.set_groups(c["groups"])
        with pytest.raises(ValueError):
            chain.set(c["logp"], *one, c["temper"])                      # and the reverse
        with pytest.raises(ValueError):
            chain.expect_grouped()                                       # before a set_grouped
        chain.set_grouped(c["glogp"], A, pi, qt, qp, c["temper"])
        with pytest.raises(ValueError):
            chain.expect()
        with pytest.raises(ValueError):
            chain.set_scan(64)                                           # the tile scan on a grouped chain
        assert np.array_equal(chain.expect_grouped()[0], c["got"]["T"])
        chain.set_groups(None)                                           # back to today's bits
        with pytest.raises(ValueError):
            chain.expect()                                               # (a set comes first)
        chain.set(c["logp"], *one, c["temper"])
        again = chain.expect(records=True), chain.decode()
        for a, b in zip(plain[0] + plain[1], again[0] + again[1]):
            assert np.array_equal(a, b)
        chain.set_scan(64)
        with pytest.raises(ValueError):
            chain.set_groups(c["groups"])                                # groups on a chain with the tile scan on
        chain.set_scan(0)
        chain.set_groups(c["groups"])
    finally:
        chain.close()
    made = _lib.Chain(ctx, np.zeros((10, 3)), [0, 4, 10], 3, emissions=True)
    try:
        with pytest.raises(ValueError):
            made.set_groups([0, 1, 2])                                   # a chain from emissions
    finally:
        made.close()


# ---- the fit ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scaffolds():
    from tests import segment_ref
    seqs = [cref.small_sequence(seed) for seed in (2, 3, 4)]
    seqs.append(segment_ref.chain_sequence(np.random.default_rng(12), cref.small_rows()[1:3], [0, 8000, 15000], 15000))
    parts = [cref.window_counts(s) for s in seqs]
    offsets = np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.uint64)
    return seqs, np.vstack(parts), offsets


def test_fit_groups_equals_fit_per_scaffold(scaffolds):
    from phamers_amd import _lib, compose
    seqs, C, offsets = scaffolds
    groups = np.arange(5, dtype=np.uint64)
    want, status = gref.fit_loop(compose, C, offsets, groups, 3)
    assert status.tolist() == [0, 0, 0, 1]
    got = compose.fit_groups(C, offsets, groups, 3)
    batch = _lib.Batch.from_counts(_lib.get_context(), C)
    try:
        resident = compose.fit_groups(batch, offsets, groups, 3)
        dec_resident = resident.decode(batch, offsets, groups)
    finally:
        batch.close()
    assert np.array_equal(got.status, status) and np.array_equal(resident.status, status)
    for g in range(4):
        gref.assert_same_composition(got[g], want[g], "scaffold %d" % g)
        gref.assert_same_composition(resident[g], want[g], "scaffold %d, resident" % g)
    dec = got.decode(C, offsets, groups)
    off = offsets.astype(int)
    for g in range(3):
        a, b = off[g], off[g + 1]
        alone_dec = want[g].decode(C[a:b], [0, b - a])
        for d in (dec, dec_resident):
            assert np.array_equal(d.state[a:b], alone_dec.state) and np.array_equal(d.posterior[a:b], alone_dec.posterior)
            assert d.log_evidence[g] == alone_dec.log_evidence[0] and d.path_score_q[g] == alone_dec.path_score_q[0]
            assert d.path_score[g] == alone_dec.path_score[0]
    assert cref.changes(dec.state[off[0]:off[1]]) == [12000, 20000, 30000]
    assert not dec.state[off[3]:].any() and np.isnan(dec.posterior[off[3]:]).all() and np.isnan(dec.log_evidence[3])


def test_segment_sequences_and_the_command_line_per_record(scaffolds, tmp_path):
    from phamers_amd import compose
    seqs, C, offsets = scaffolds
    result = compose.segment_sequences(seqs, 3, per_record=True)
    comps = result.composition
    assert isinstance(comps, compose.Compositions) and comps.status.tolist() == [0, 0, 0, 1] and len(result) == len(C)
    first = [r for r in result.regions() if r[0] == result.record_ids[0]]
    assert [r[2] for r in first] == [12000, 20000, 30000, 40000]
    alone = compose.segment_sequences(seqs[:1], 3)
    assert np.array_equal(alone.state, result.state[:80]) and np.array_equal(alone.composition.log_profiles, comps[0].log_profiles)
    fasta, out = str(tmp_path / "assembly.fasta"), str(tmp_path / "out")
    with open(fasta, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">scaffold%d\n%s\n" % (i, "\n".join(s[j:j + 80] for j in range(0, len(s), 80))))
    cli = compose.main(["-in", fasta, "-out", out, "-S", "3", "--per_record"])
    assert np.array_equal(cli.state, result.state) and np.array_equal(cli.composition.log_profiles, comps.log_profiles, equal_nan=True)
    assert sorted(os.listdir(out)) == ["compose_profiles.csv", "compose_records.csv", "compose_segments.csv", "compose_trace.csv",
                                       "compose_windows.csv"]
    records = list(csv.DictReader(open(os.path.join(out, "compose_records.csv"))))
    assert [r["record_id"] for r in records] == ["scaffold%d" % i for i in range(4)]
    assert [int(r["n_windows"]) for r in records] == [80, 80, 80, 30] and [int(r["status"]) for r in records] == [0, 0, 0, 1]
    assert [int(r["n_iter"]) for r in records] == comps.n_iter.tolist()
    profiles = list(csv.DictReader(open(os.path.join(out, "compose_profiles.csv"))))
    assert [(p["record_id"], p["state"]) for p in profiles] == [("scaffold%d" % i, str(s)) for i in range(3) for s in range(3)]
    segments = [s for s in csv.DictReader(open(os.path.join(out, "compose_segments.csv"))) if s["record_id"] == "scaffold0"]
    assert [int(s["end"]) for s in segments] == [12000, 20000, 30000, 40000]
    with pytest.raises(SystemExit):
        compose.main(["-in", fasta, "-out", out, "-S", "3", "--per_record", "--scan"])
