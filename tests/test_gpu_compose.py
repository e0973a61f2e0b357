"""GPU: the S-state chain over window count rows (chain.hip) and the fit around it (phamers_amd/compose.py) against the
statement of tests/compose_ref.py: emissions within their dot-product bound and bit-equal across entry points and batch
splits, the Viterbi path bit for bit the integer recurrence on the device's own emissions, posteriors / evidence / expected
counts within the derived bounds of the sequential longdouble statement, independence of a record from the rest of the
call, exact ties, extremes, error codes, the fit and the command line on the "small" sequence.  Shapes are the smallest that
reach each path: records of 1, 2, 63, 64, 65, 129 and 1000 windows with an empty and a one-window record among them (1325
rows: two reduction blocks of 1024, eleven emission tiles of 128), S = 2 .. 8 (every state count: the padded widths 2, 4 and
8 full, and with one, two and three padded lanes), D = 256 and a D that is no multiple of 4 (S = 3, 4 and 8).  The shapes
past these -- launches, tile counts, fold levels, column groups -- are tests/test_gpu_chain_shapes.py's."""
import csv
import os

import numpy as np
import pytest

from tests import compose_ref as cref, helpers

pytestmark = pytest.mark.gpu
LD = cref.LD
LENGTHS = [1, 2, 63, 0, 64, 65, 129, 1, 1000]
STATES = [2, 3, 4, 5, 6, 7, 8]


def chain_parameters(rng, S, stay=0.9):
    A = np.full((S, S), (1.0 - stay) / (S - 1)) * (0.5 + rng.random((S, S)))
    np.fill_diagonal(A, 0.0)
    np.fill_diagonal(A, 1.0 - A.sum(axis=1))
    pi = 0.2 + rng.random(S)
    A, pi = A / A.sum(axis=1, keepdims=True), pi / pi.sum()
    return A, pi, cref.quantise_log(A), cref.quantise_log(pi)


def make_case(S, D, seed=0, kmers=60, lengths=LENGTHS):
    """Count rows drawn along a sticky path from S nearby profiles, the (slightly wrong) log profiles, a chain."""
    rng = np.random.default_rng(1000 * S + D + seed)
    base = rng.dirichlet(np.full(D, 5.0))
    profiles = np.array([(lambda p: p / p.sum())(base * np.exp(0.35 * rng.standard_normal(D))) for _ in range(S)])
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    n = int(offsets[-1])
    state = (np.arange(n) // 23 + rng.integers(0, S)) % S
    counts = np.vstack([rng.multinomial(kmers, profiles[s]) for s in state]).astype(np.uint32)
    counts[rng.choice(n, max(1, n // 50), replace=False)] = 0          # windows without k-mers inside records
    logp = np.log((lambda p: p / p.sum(axis=1, keepdims=True))(profiles * np.exp(0.05 * rng.standard_normal((S, D)))))
    return dict(S=S, D=D, counts=counts, offsets=offsets, logp=logp, par=chain_parameters(rng, S), temper=0.75)


def run(case, batch_rows=0, resident=False, emissions=None, offsets=None):
    """dict of everything the device returns for a case (or for host emissions)."""
    from phamers_amd import _lib
    ctx = _lib.get_context()
    A, pi, qt, qp = case["par"]
    off = case["offsets"] if offsets is None else offsets
    batch = _lib.Batch.from_counts(ctx, case["counts"]) if resident else None
    assert not resident or batch is not None
    if emissions is not None:
        chain = _lib.Chain(ctx, emissions, off, case["S"], emissions=True)
    else:
        chain = _lib.Chain(ctx, batch if resident else case["counts"], off, case["S"], batch_rows)
    try:
        chain.set(None if emissions is not None else case["logp"], A, pi, qt, qp, case["temper"])
        out = dict(E=chain.emissions())
        out["T"], out["Ns"], out["xi"], out["gamma0"], out["L"], out["L_rec"] = chain.expect(records=True)
        out["state"], out["posterior"], out["le"], out["score"] = chain.decode()
    finally:
        chain.close()
        if batch is not None:
            batch.close()
    return out


def same(a, b, keys=("E", "T", "Ns", "xi", "gamma0", "L", "L_rec", "state", "posterior", "le", "score")):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in keys if a[k] is not None)


@pytest.fixture(scope="module")
def cases():
    out = {(S, 256): make_case(S, 256) for S in STATES}
    for S in (3, 4, 8):
        out[(S, 30)] = make_case(S, 30)
    for c in out.values():
        c["got"] = run(c)
    return out


KEYS = [(S, 256) for S in STATES] + [(3, 30), (4, 30), (8, 30)]


@pytest.mark.parametrize("key", KEYS)
def test_emissions_within_their_bound(cases, key):
    c = cases[key]
    exact = cref.exact_emissions(c["counts"], c["logp"], c["temper"])
    err = np.abs(c["got"]["E"].astype(LD) - exact).astype(np.float64)
    bound = cref.emission_bound(c["counts"], c["logp"], c["temper"])
    print("emissions %r: worst error / bound %.3g" % (key, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    zero = c["counts"].sum(axis=1) == 0
    assert zero.any() and (c["got"]["E"][zero] == 0.0).all()          # no k-mers: E = 0 for every state


@pytest.mark.parametrize("S", STATES)
def test_same_bits_from_host_rows_a_resident_batch_and_any_batch_rows(cases, S):
    c = cases[(S, 256)]
    assert len(c["counts"]) > 1024                                     # the default takes one batch, batch_rows = 1024 two
    for kw in (dict(batch_rows=1024), dict(resident=True), dict(resident=True, batch_rows=1000), dict()):
        assert same(c["got"], run(c, **kw)), kw
    assert same(cases[(3, 30)]["got"], run(cases[(3, 30)], batch_rows=1))


@pytest.mark.parametrize("key", KEYS)
def test_viterbi_is_the_integer_recurrence_on_the_devices_own_emissions(cases, key):
    c, got = cases[key], cases[key]["got"]
    A, pi, qt, qp = c["par"]
    states, scores = cref.viterbi_records(got["E"], c["offsets"], qt, qp)
    assert np.array_equal(got["state"], states) and got["score"].tolist() == scores
    assert len(set(states.tolist())) == c["S"]                          # the path visits every state


@pytest.mark.parametrize("S", [2, 3])
def test_short_records_against_the_brute_force(S):
    rng = np.random.default_rng(40 + S)
    lengths = [1, 2, 3, 4, 5, 6, 7, 7]
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    E = rng.normal(0.0, 2.5, (int(offsets[-1]), S))
    case = dict(S=S, par=chain_parameters(rng, S, 0.7), temper=1.0, offsets=offsets)
    got = run(case, emissions=E)
    A, pi, qt, qp = case["par"]
    assert np.array_equal(got["E"], E) and got["T"] is None
    for r, (a, b) in enumerate(zip(offsets[:-1].astype(int), offsets[1:].astype(int))):
        gamma, xi, le, best, paths = cref.brute_force(E[a:b], A, pi, qt, qp)
        assert got["score"][r] == best and tuple(got["state"][a:b].tolist()) in paths
        cref.check_posterior(got["posterior"][a:b], gamma, b - a, S, "record %d" % r)
        assert abs(LD(got["le"][r]) - le) <= cref.evidence_bound(E[a:b].max(axis=1), S, le)


@pytest.mark.parametrize("key", KEYS)
def test_posteriors_evidence_and_expected_counts_within_the_derived_bounds(cases, key):
    c, got = cases[key], cases[key]["got"]
    S, off = c["S"], c["offsets"].astype(int)
    A, pi = c["par"][:2]
    n, R, longest = len(c["counts"]), len(off) - 1, int(np.diff(off).max())
    want = cref.expect(got["E"], off, A, pi, c["counts"])
    worst = cref.check_posterior(got["posterior"], want["gamma"], longest, S, "posterior")
    print("posterior %r: worst error / bound %.3g" % (key, worst))
    M = got["E"].max(axis=1)
    for r in range(R):
        b = cref.evidence_bound(M[off[r]:off[r + 1]], S, want["log_evidence_rec"][r])
        assert abs(LD(got["le"][r]) - want["log_evidence_rec"][r]) <= b, r
    assert np.array_equal(got["le"], got["L_rec"])                      # decode and expect: the same forward pass
    total = sum(cref.evidence_bound(M[off[r]:off[r + 1]], S, want["log_evidence_rec"][r]) for r in range(R))
    total += R * cref.U * float(np.abs(want["log_evidence_rec"]).sum())
    assert abs(LD(got["L"]) - want["log_evidence"]) <= total
    cref.check_sums(got["xi"], want["xi"], longest, S, n + R, n, "xi")
    cref.check_sums(got["gamma0"], want["gamma0"], longest, S, R, R, "gamma0")
    cref.check_sums(got["T"], want["T"], longest, S, n, float(c["counts"].sum()), "T")
    cref.check_sums(got["Ns"], want["Ns"], longest, S, n, n, "Ns")
    # the sum rules, within the same bounds
    B = cref.posterior_bound(longest, S)
    assert np.abs(got["posterior"].sum(axis=1) - 1.0).max() <= B + S * cref.U
    nonempty = int((np.diff(off) > 0).sum())
    assert abs(got["xi"].sum() - (n - nonempty)) <= (B + (n + R + 2) * cref.U) * n
    assert abs(got["gamma0"].sum() - nonempty) <= (B + (R + 2) * cref.U) * R
    col = c["counts"].sum(axis=0, dtype=np.uint64).astype(np.float64)
    assert (np.abs(got["T"].sum(axis=0) - col) <= (B + (n + S + 2) * cref.U) * col).all()
    assert (np.abs(got["Ns"] - got["posterior"].sum(axis=0)) <= (B + (2 * n + 2) * cref.U) * n).all()


@pytest.mark.parametrize("S", [3, 8])
def test_a_record_alone_gives_the_bits_it_gives_inside_a_shuffled_call(cases, S):
    c = cases[(S, 256)]
    got = run(c)
    assert same(c["got"], got)                                          # two runs are identical
    off = c["offsets"].astype(int)
    order = np.random.default_rng(S).permutation(len(off) - 1)
    rows = np.concatenate([np.arange(off[r], off[r + 1]) for r in order]).astype(int)
    shuffled = dict(c, counts=c["counts"][rows], offsets=np.concatenate(([0], np.cumsum(np.diff(off)[order]))).astype(np.uint64))
    sh = run(shuffled)
    at = shuffled["offsets"].astype(int)
    for i, r in enumerate(order):
        a, b, sa, sb = off[r], off[r + 1], at[i], at[i + 1]
        for k in ("E", "state", "posterior"):
            assert np.array_equal(got[k][a:b], sh[k][sa:sb]), (k, r)
        assert got["le"][r] == sh["le"][i] and got["score"][r] == sh["score"][i]
        alone = run(dict(c, counts=c["counts"][a:b], offsets=np.array([0, b - a], dtype=np.uint64)))
        for k in ("E", "state", "posterior"):
            assert np.array_equal(got[k][a:b], alone[k]), (k, r)
        assert got["le"][r] == alone["le"][0] and got["score"][r] == alone["score"][0]


@pytest.mark.parametrize("S,extra", [(2, 300), (4, 600), (5, 900)])
def test_more_records_than_one_launch_covers(S, extra):
    from phamers_amd import _lib
    pad = 2 if S <= 2 else (4 if S <= 4 else 8)
    R = int(_lib.load().phk_chain_grid_pass()) * 2 // pad + extra      # records one launch covers at this width, and more
    rng = np.random.default_rng(S)
    lengths = rng.integers(0, 4, R)
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    E = rng.normal(0.0, 2.0, (int(offsets[-1]), S))
    case = dict(S=S, par=chain_parameters(rng, S, 0.8), temper=1.0, offsets=offsets)
    got = run(case, emissions=E)
    A, pi, qt, qp = case["par"]
    states, scores = cref.viterbi_records(E, offsets, qt, qp)
    assert np.array_equal(got["state"], states) and got["score"].tolist() == scores
    for lo, hi in ((0, 200), (R - 200, R)):                              # the first records and those past the launch, alone
        a, b = int(offsets[lo]), int(offsets[hi])
        part = run(case, emissions=E[a:b], offsets=offsets[lo:hi + 1] - offsets[lo])
        assert np.array_equal(part["posterior"], got["posterior"][a:b]) and np.array_equal(part["le"], got["le"][lo:hi])
        assert np.array_equal(part["state"], got["state"][a:b]) and np.array_equal(part["score"], got["score"][lo:hi])
    n, nonempty = len(E), int((lengths > 0).sum())
    B = cref.posterior_bound(3, S)
    assert abs(got["xi"].sum() - (n - nonempty)) <= (B + (n + R + 2) * cref.U) * n
    assert abs(got["gamma0"].sum() - nonempty) <= (B + (R + 2) * cref.U) * R
    assert abs(got["L"] - got["le"].astype(LD).sum()) <= R * cref.U * np.abs(got["le"]).sum() + 1e-300


def test_exact_ties():
    rng = np.random.default_rng(9)
    S, D, n = 3, 256, 70
    counts = rng.multinomial(80, rng.dirichlet(np.ones(D)), n).astype(np.uint32)
    row = np.log(rng.dirichlet(np.full(D, 3.0)))
    A = np.full((S, S), 0.05)
    np.fill_diagonal(A, 0.9)
    pi = np.full(S, 1.0 / 3.0)
    par = (A, pi, cref.quantise_log(A), cref.quantise_log(pi))
    case = dict(S=S, counts=counts, logp=np.tile(row, (S, 1)), par=par, temper=1.0, offsets=np.array([0, n], dtype=np.uint64))
    got = run(case)
    assert (got["E"] == got["E"][:, :1]).all()                          # equal profiles: equal bits in every state
    assert (got["state"] == 0).all() and np.abs(got["posterior"] - 1.0 / 3.0).max() <= cref.posterior_bound(n, S)
    # two equal states beside a worse one: the tie rule decides, as in the statement
    other = np.log(rng.dirichlet(np.full(D, 3.0)))
    case2 = dict(case, logp=np.vstack([other, row, row]))
    counts2 = rng.multinomial(80, np.exp(row), n).astype(np.uint32)
    got2 = run(dict(case2, counts=counts2))
    states, scores = cref.viterbi_records(got2["E"], case["offsets"], par[2], par[3])
    assert np.array_equal(got2["state"], states) and (got2["state"] == 1).all() and got2["score"].tolist() == scores
    # (their posteriors are equal in exact arithmetic; the two lanes add their terms in another order)
    assert np.abs(got2["posterior"][:, 1] - got2["posterior"][:, 2]).max() <= 2 * cref.posterior_bound(n, S)


@pytest.mark.parametrize("S", [2, 5])
def test_extremes(S):
    rng = np.random.default_rng(70 + S)
    n = 130
    offsets = np.array([0, n], dtype=np.uint64)
    # emission gaps of 1e5 nats, the favoured state changing every 9 windows; transitions at 1e-12
    E = np.full((n, S), -1e5) * (0.5 + 0.5 * rng.random((n, S)))
    E[np.arange(n), (np.arange(n) // 9) % S] = 0.0
    A = np.full((S, S), 1e-12)
    np.fill_diagonal(A, 1.0 - (S - 1) * 1e-12)
    pi = np.full(S, 1.0 / S)
    pi[0] = 1.0 - pi[1:].sum()
    case = dict(S=S, par=(A, pi, cref.quantise_log(A), cref.quantise_log(pi)), temper=1.0, offsets=offsets)
    got = run(case, emissions=E)
    for k in ("posterior", "le", "xi", "gamma0", "L"):
        assert np.isfinite(got[k]).all(), k
    assert (got["posterior"].max(axis=1) >= 1.0 - 1e-9).all()              # certain states
    want = cref.expect(E, offsets, A, pi)
    cref.check_posterior(got["posterior"], want["gamma"], n, S, "extremes")
    assert abs(LD(got["le"][0]) - want["log_evidence_rec"][0]) <= cref.evidence_bound(E.max(axis=1), S, want["log_evidence_rec"][0])
    states, scores = cref.viterbi_records(E, offsets, case["par"][2], case["par"][3])
    assert np.array_equal(got["state"], states) and got["score"].tolist() == scores
    assert np.array_equal(got["state"], (np.arange(n) // 9) % S)


def test_errors_come_before_any_launch_and_leave_the_next_call_alone(cases):
    from phamers_amd import _lib
    ctx = _lib.get_context()
    c = cases[(3, 256)]
    A, pi, qt, qp = c["par"]
    counts, off = c["counts"], c["offsets"]
    for S in (1, 9):
        with pytest.raises(ValueError):
            _lib.Chain(ctx, counts, off, S)
    for bad in (off[::-1].copy(), np.concatenate((off[:-1], [off[-1] + 1])), np.concatenate(([1], off[1:]))):
        with pytest.raises(ValueError):
            _lib.Chain(ctx, counts, bad.astype(np.uint64), 3)
    with pytest.raises(ValueError):
        _lib.Chain(ctx, np.full((4, 3), np.nan), [0, 4], 3, emissions=True)
    with pytest.raises(ValueError):
        _lib.Chain(ctx, np.full((4, 3), np.inf), [0, 4], 3, emissions=True)
    chain = _lib.Chain(ctx, counts, off, 3)
    try:
        with pytest.raises(ValueError):
            chain.expect()                                               # before a set
        def refused(**kw):
            a = dict(log_profiles=c["logp"], trans=A, init=pi, qlog_trans=qt, qlog_init=qp, temper=c["temper"])
            a.update(kw)
            with pytest.raises(ValueError):
                chain.set(**a)
        A0, A1, As = A.copy(), A.copy(), A.copy()
        A0[1, 2], A1[0, 0], As[2] = 0.0, 1.0, As[2] * (1 + 1e-12)
        p0, ps = pi.copy(), pi * (1 - 1e-12)
        p0[0] = 0.0
        for kw in (dict(trans=A0), dict(trans=A1), dict(trans=As), dict(init=p0), dict(init=ps), dict(temper=0.0),
                   dict(temper=np.inf), dict(temper=np.nan), dict(log_profiles=c["logp"][:, :-4]), dict(qlog_trans=-qt - 1)):
            refused(**kw)
        lp = c["logp"].copy()
        lp[1, 7] = -np.inf
        refused(log_profiles=lp)                                         # PHK_ERR_NAN
        lp[1, 7] = np.nan
        refused(log_profiles=lp)
        with pytest.raises(ValueError):
            chain.decode()                                               # the failed sets left no parameters behind
        chain.set(c["logp"], A, pi, qt, qp, c["temper"])
        out = chain.expect(records=True)
        state, post, le, score = chain.decode()
    finally:
        chain.close()
    got = c["got"]
    assert np.array_equal(out[0], got["T"]) and np.array_equal(out[2], got["xi"]) and out[4] == got["L"]
    assert np.array_equal(state, got["state"]) and np.array_equal(post, got["posterior"]) and np.array_equal(score, got["score"])
    # nothing to do is no error
    for n_off in ([0], [0, 0, 0]):
        empty = _lib.Chain(ctx, np.zeros((0, 256), dtype=np.uint32), n_off, 3)
        empty.set(c["logp"], A, pi, qt, qp, 1.0)
        T, Ns, xi, g0, L = empty.expect()
        st, po, le0, sc = empty.decode()
        empty.close()
        assert not T.any() and not Ns.any() and not xi.any() and not g0.any() and L == 0.0
        assert len(st) == 0 and not le0.any() and not sc.any() and len(le0) == len(n_off) - 1


# ---- the fit and the command line on the "small" sequence ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    seq = cref.small_sequence(2)
    return seq, cref.window_counts(seq)


def test_fit_on_the_small_sequence(small, monkeypatch):
    from phamers_amd import compose
    seq, C = small
    off = [0, len(C)]
    comp = compose.fit(C, off, 3)
    # F never falls by more than the rounding of the evidence (the profiles' part of F is exact to a few u of its size)
    M = np.abs(C.astype(np.float64) @ comp.log_profiles.T).max(axis=1)
    slack = 2 * cref.evidence_bound(M, 3, comp.trace[-1, 0]) + 16 * cref.U * abs(comp.trace[-1, 1])
    print("fit: F per iterate %r, slack %.3g" % (comp.trace[:, 1].tolist(), slack))
    assert (np.diff(comp.trace[:, 1]) >= -slack).all() and comp.converged
    dec = comp.decode(C, off)
    assert cref.changes(dec.state) == [12000, 20000, 30000] and dec.state[0] == dec.state[-1]
    from phamers_amd import _lib
    batch = _lib.Batch.from_counts(_lib.get_context(), C)
    try:
        resident = compose.fit(batch, off, 3)
    finally:
        batch.close()
    assert np.array_equal(resident.log_profiles, comp.log_profiles) and np.array_equal(resident.trans, comp.trans)
    monkeypatch.setattr(compose, "_estep", cref.StatementEStep)
    want = compose.fit(C, off, 3)
    assert want.n_iter == comp.n_iter
    assert np.abs(np.diag(want.trans) - np.diag(comp.trans)).max() <= 1e-9


def test_command_line_end_to_end(small, tmp_path):
    from phamers_amd import compose, fileIO
    seq, C = small
    g = helpers.load_npz("ref_features.npz")
    pos = np.delete(g["pos_counts"].astype(np.int64), 2200, axis=0)
    neg = np.delete(g["neg_counts"].astype(np.int64), [100, 2000], axis=0)
    fasta, out = str(tmp_path / "genome.fasta"), str(tmp_path / "out")
    with open(fasta, "w") as f:
        f.write(">genome\n" + "\n".join(seq[i:i + 80] for i in range(0, len(seq), 80)) + "\n")
    fileIO.save_counts(pos, ["p%d" % i for i in range(len(pos))], str(tmp_path / "pos.csv"))
    fileIO.save_counts(neg, ["n%d" % i for i in range(len(neg))], str(tmp_path / "neg.csv"))
    result = compose.main(["-in", fasta, "-out", out, "-S", "3", "-pf", str(tmp_path / "pos.csv"), "-nf", str(tmp_path / "neg.csv")])
    assert len(result) == 80 and result.composition.temper == 1.0
    for name in ("compose_windows.csv", "compose_segments.csv", "compose_profiles.csv", "compose_trace.csv"):
        assert os.path.getsize(os.path.join(out, name)) > 0, name
    segments = list(csv.DictReader(open(os.path.join(out, "compose_segments.csv"))))
    assert [int(s["end"]) for s in segments] == [12000, 20000, 30000, 40000]
    assert [int(s["start"]) for s in segments] == [0, 12000, 20000, 30000] and segments[0]["state"] == segments[3]["state"]
    assert all(s["record_id"] == "genome" for s in segments) and sum(int(s["n_windows"]) for s in segments) == 80
    profiles = list(csv.DictReader(open(os.path.join(out, "compose_profiles.csv"))))
    score = {p["state"]: float(p["phage_score"]) for p in profiles}
    assert len(score) == 3 and np.isfinite(list(score.values())).all()
    assert [s for s, v in score.items() if v > 0] == [segments[1]["state"]]       # only the second piece's state is phage
    windows = list(csv.DictReader(open(os.path.join(out, "compose_windows.csv"))))
    assert len(windows) == 80 and [int(w["start"]) for w in windows] == list(range(0, 40000, 500))
    assert abs(sum(float(windows[0]["posterior%d" % s]) for s in range(3)) - 1.0) < 1e-12
    assert len(list(csv.DictReader(open(os.path.join(out, "compose_trace.csv"))))) == result.composition.n_iter + 1
