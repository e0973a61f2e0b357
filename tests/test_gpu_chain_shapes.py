"""GPU: the S-state chain (chain.hip, DESIGN.md sections 4.26 - 4.28) past the shapes the fixtures of tests/test_gpu_compose.py,
tests/test_gpu_chain_scan.py and tests/test_gpu_compose_groups.py reach, against the same statements and the same derived
bounds (tests/compose_ref.py, tests/chain_scan_ref.py, tests/compose_groups_ref.py; no tolerance of this file's own):

    more scanned records than one launch of the carry covers (its stride starts at 16 CB + 1, 4 CB + 1 and CB + 1 records at
      the widths 2, 4 and 8, CB = phk_chain_grid_pass() / 32), of the kernel of the tile ends (64 CB + 1) and of the fold of
      the tiles' xi (ns S^2 > 4096 * 256): S = 3, 8, 2 with 4 CB + 300, 16 CB + 300 and 64 CB + 300 records of 1, 2, 3 and
      T + 1 windows
    every tile count K = 1 .. 20 of a scanned record, with a last tile of one window and with a full last tile, in one call:
      the carry keeps a fixed number of tiles in registers and refills a slot with the tile that many ahead, behind three
      differently written guards
    a group whose fold has two and three levels over its records' vectors (300 and 256^2 + 1 records) and two over its row
      blocks' vectors (257 blocks of 1024 windows), between groups that have one, in one batch and cut into several
    one chain under a sequence of active masks and parameters: the descriptor tables follow the mask, the buffers are reused
    D = 320 (two column groups of 256, the second partial), D = 16 (vector loads, no full K step) and D = 1024 (four groups)
    emissions from the host past one pass of the row maximum kernel (4096 workgroups of 256 rows)
    ``Chain.decode(posterior=False)`` on the three routes
"""
import numpy as np
import pytest

from tests import chain_scan_ref as sref, compose_groups_ref as gref, compose_ref as cref
from tests import test_gpu_chain_scan as scan, test_gpu_compose as base, test_gpu_compose_groups as groups

pytestmark = pytest.mark.gpu
LD, U = cref.LD, cref.U
T = sref.TILE
ROWMAX_PASS = 4096 * 256       # rows one pass of phk_chain_rowmax_kernel covers (chain.hip: 4096 workgroups of 256 rows)


def sums_ratio(got, exact, n_longest, S, terms, floor_terms, what):
    """``compose_ref.check_sums``, and the worst error over that bound for the report."""
    cref.check_sums(got, exact, n_longest, S, terms, floor_terms, what)
    exact = np.asarray(exact, dtype=LD)
    bound = LD(cref.posterior_bound(n_longest, S) + (terms + 2.0) * U) * exact + LD(cref.FLOOR) * LD(floor_terms)
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - exact)
    return float((err / np.maximum(bound, LD(1e-4000))).max()) if err.size else 0.0


# ---- 1: more scanned records than one launch of the carry, of the ends and of the xi fold -------------------------------------
@pytest.mark.parametrize("S,times", [(3, 4), (8, 16), (2, 64)])
def test_more_scanned_records_than_one_carry_launch(S, times):
    from phamers_amd import _lib
    assert int(_lib.load().phk_chain_tile()) == T
    CB = int(_lib.load().phk_chain_grid_pass()) // 32                       # the workgroups of one launch
    R = times * CB + 300
    rng = np.random.default_rng(100 + S)
    lengths = rng.choice([1, 2, 3], R)
    lengths[rng.choice(R, R // 100, replace=False)] = T + 1               # two tiles: the carry, the ends and the fold have a step
    lengths[[3, 150, R - 150, R - 3]] = T + 1
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    off, n = offsets.astype(np.int64), int(offsets[-1])
    E = rng.normal(0.0, 2.0, (n, S))
    case = dict(S=S, par=base.chain_parameters(rng, S, 0.8), temper=1.0, offsets=offsets)
    A, pi, qt, qp = case["par"]
    got = scan.run(case, 1, emissions=E)                                  # every record has a window: every record is scanned
    seq = scan.run(case, 0, emissions=E, expect=False)
    states, scores = cref.viterbi_records(E, offsets, qt, qp)
    assert np.array_equal(got["state"], states) and got["score"].tolist() == scores
    assert np.array_equal(got["state"], seq["state"]) and np.array_equal(got["score"], seq["score"])
    # the float results against the per-record route, record by record: within B + B_scan, which depend on the length alone
    rec_of = np.repeat(np.arange(R), lengths)
    worst = 0.0
    for length in (1, 2, 3, T + 1):
        rows = np.flatnonzero(lengths[rec_of] == length)
        worst = max(worst, sref.check_posterior(got["posterior"][rows], seq["posterior"][rows].astype(LD), length, S,
                                                "records of %d windows" % length, extra=cref.posterior_bound(length, S)))
    M = E.max(axis=1)
    for r in range(R):
        m = M[off[r]:off[r + 1]]
        both = sref.scan_evidence_bound(m, S, seq["le"][r]) + cref.evidence_bound(m, S, seq["le"][r])
        assert abs(LD(got["le"][r]) - LD(seq["le"][r])) <= both, r
    assert np.array_equal(got["le"], got["L_rec"])
    # the first records and those past every launch, in calls of their own
    for lo, hi in ((0, 200), (R - 200, R)):
        a, b = int(off[lo]), int(off[hi])
        part_off = offsets[lo:hi + 1] - offsets[lo]
        part = scan.run(case, 1, emissions=E[a:b], offsets=part_off, expect=False)
        assert (lengths[lo:hi] > T).sum() >= 2
        for r in range(lo, hi):
            assert scan.record_equal(got, part, off, r, part_off, r - lo), r
    B = sref.scan_posterior_bound(T + 1, S)
    xi_err, g0_err = abs(got["xi"].sum() - (n - R)), abs(got["gamma0"].sum() - R)
    print("S = %d, %d scanned records: worst distance from the per-record route / (B + B_scan) %.3g, xi sum rule %.3g, gamma_0 "
          "sum rule %.3g of their bounds" % (S, R, worst, xi_err / ((B + (n + R + 2) * U) * n), g0_err / ((B + (R + 2) * U) * R)))
    assert xi_err <= (B + (n + R + 2) * U) * n
    assert g0_err <= (B + (R + 2) * U) * R
    assert abs(got["L"] - got["le"].astype(LD).sum()) <= R * U * np.abs(got["le"]).sum()


# ---- 2: every tile count around the carry's look-ahead -----------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 5, 8])
def test_every_tile_count_around_the_carry_look_ahead(S):
    # The carry holds 8 tiles today and refills a slot with the tile 8 ahead.  The depth is not exported, so the records
    # cover K = 1 .. 20 whatever it is below 10: for a depth of 8 that is two refills of every slot and every value of
    # the three guards (tn < t1, cn + 1 < K, p + 1 < K) on both sides of the edges K = 8, 9, 16, 17.
    lengths = [n for K in range(1, 21) for n in ((K - 1) * T + 1, K * T)]
    c = base.make_case(S, 30, seed=5, lengths=lengths)
    off = c["offsets"].astype(int)
    R, n = len(lengths), int(off[-1])
    A, pi, qt, qp = c["par"]
    got, seq = scan.run(c, 1), scan.run(c, 0, expect=False)
    assert np.array_equal(got["E"], seq["E"])
    states, scores = cref.viterbi_records(got["E"], c["offsets"], qt, qp)
    assert np.array_equal(got["state"], states) and got["score"].tolist() == scores
    assert np.array_equal(got["state"], seq["state"]) and np.array_equal(got["score"], seq["score"])
    assert len(set(states.tolist())) == S
    want = cref.expect(got["E"], off, A, pi, c["counts"])
    M = got["E"].max(axis=1)
    worst = dict(posterior=0.0, evidence=0.0)
    for r in range(R):
        a, b = off[r], off[r + 1]
        worst["posterior"] = max(worst["posterior"], sref.check_posterior(got["posterior"][a:b], want["gamma"][a:b], b - a, S,
                                                                          "posterior of record %d" % r))
        worst["evidence"] = max(worst["evidence"], sref.check_evidence(got["le"][r], want["log_evidence_rec"][r], M[a:b], S,
                                                                       "record %d" % r))
    assert np.array_equal(got["le"], got["L_rec"])
    total = sum(sref.scan_evidence_bound(M[off[r]:off[r + 1]], S, want["log_evidence_rec"][r]) for r in range(R))
    total += R * U * float(np.abs(want["log_evidence_rec"]).sum())
    assert abs(LD(got["L"]) - want["log_evidence"]) <= total
    longest = max(lengths)
    worst["xi"] = sref.check_sums(got["xi"], want["xi"], longest, S, n + R, n, "xi")
    worst["gamma0"] = sref.check_sums(got["gamma0"], want["gamma0"], longest, S, R, R, "gamma0")
    worst["T"] = sref.check_sums(got["T"], want["T"], longest, S, n, float(c["counts"].sum()), "T")
    worst["Ns"] = sref.check_sums(got["Ns"], want["Ns"], longest, S, n, n, "Ns")
    print("tile counts 1 .. 20, S = %d: worst error / bound %s" % (S, ", ".join("%s %.3g" % kv for kv in worst.items())))
    for r in range(R):                                                    # every record in a call of its own
        a, b = off[r], off[r + 1]
        alone = scan.run(dict(c, counts=c["counts"][a:b], offsets=np.array([0, b - a], dtype=np.uint64)), 1, expect=False)
        assert scan.record_equal(got, alone, off, r, [0, b - a], 0), (r, lengths[r])


# ---- 3: a group's fold past one level ------------------------------------------------------------------------------------------
def fold_case():
    """S = 2, D = 12 (neither vector loads nor a full K step).  Five groups: 3 records; 300 records of 1 - 3 windows (two
    levels over the records' vectors); 256^2 + 1 one-window records (three); 256 * 1024 / 64 + 5 records of 64 windows (257
    row blocks: two levels over the blocks' vectors, and two over the records'); 2 records.  The rows are runs of consecutive
    windows of one ``make_case`` path."""
    S, D, pool = 2, 12, 4096
    src = base.make_case(S, D, seed=11, lengths=[pool])
    rng = np.random.default_rng(31)
    per_group = [np.array([5, 0, 70]), rng.integers(1, 4, 300), np.ones(256 * 256 + 1, dtype=np.int64),
                 np.full(256 * 1024 // 64 + 5, 64), np.array([3, 1])]
    lengths = np.concatenate(per_group).astype(np.int64)
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    rec_of = np.repeat(np.arange(len(lengths)), lengths)
    at = np.arange(int(offsets[-1])) - offsets.astype(np.int64)[rec_of]
    counts = np.ascontiguousarray(src["counts"][(rng.integers(0, pool, len(lengths))[rec_of] + at) % pool])
    G = len(per_group)
    logp = np.array([np.log((lambda p: p / p.sum(axis=1, keepdims=True))(np.exp(src["logp"] + 0.2 * rng.standard_normal((S, D)))))
                     for _ in range(G)])
    par = [base.chain_parameters(rng, S, 0.6 + 0.35 * rng.random()) for _ in range(G)]
    group_offsets = np.concatenate(([0], np.cumsum([len(p) for p in per_group]))).astype(np.uint64)
    return dict(src, counts=counts, offsets=offsets, groups=group_offsets, glogp=logp, gpar=par)


def check_statement(c, part, g):
    """Group g's part against the statement, as tests/test_gpu_compose_groups.py checks every group of its fixture."""
    rows, off = gref.group_rows(c["counts"], c["offsets"], c["groups"], g)
    S, off = c["S"], off.astype(int)
    A, pi, qt, qp = c["gpar"][g]
    n, R = len(rows), len(off) - 1
    states, scores = cref.viterbi_records(part["E"], off, qt, qp)
    assert np.array_equal(part["state"], states) and part["score"].tolist() == scores, g
    exact = cref.exact_emissions(rows, c["glogp"][g], c["temper"])
    assert (np.abs(part["E"].astype(LD) - exact).astype(np.float64) <= cref.emission_bound(rows, c["glogp"][g], c["temper"])).all()
    longest = int(np.diff(off).max())
    want = cref.expect(part["E"], off, A, pi, rows)
    worst = cref.check_posterior(part["posterior"], want["gamma"], longest, S, "posterior of group %d" % g)
    M = part["E"].max(axis=1)
    total = LD(0)
    for r in range(R):
        b = cref.evidence_bound(M[off[r]:off[r + 1]], S, want["log_evidence_rec"][r])
        assert abs(LD(part["le"][r]) - want["log_evidence_rec"][r]) <= b, (g, r)
        total += b
    total += R * U * float(np.abs(want["log_evidence_rec"]).sum())
    assert abs(LD(part["L"]) - want["log_evidence"]) <= total, g
    return max(worst, sums_ratio(part["xi"], want["xi"], longest, S, n + R, n, "xi"),
               sums_ratio(part["gamma0"], want["gamma0"], longest, S, R, R, "gamma0"),
               sums_ratio(part["T"], want["T"], longest, S, n, float(rows.sum()), "T"),
               sums_ratio(part["Ns"], want["Ns"], longest, S, n, n, "Ns"))


def test_group_folds_past_one_level():
    c = fold_case()
    S, G = c["S"], len(c["groups"]) - 1
    spans = gref.group_spans(c["offsets"], c["groups"])
    records, windows = [s[1] - s[0] for s in spans], [s[3] - s[2] for s in spans]
    assert 256 < records[1] <= 256 ** 2 < records[2] and 256 < records[3] <= 256 ** 2 and -(-windows[3] // 1024) == 257
    assert max(records[0], records[4]) <= 256 and max(-(-w // 1024) for w in windows[:3] + windows[4:]) <= 256
    alone = [groups.alone(c, g) for g in range(G)]                         # (the ungrouped fold past one level too)
    several = 100 * 1024
    assert windows[3] > 2 * several
    lengths = np.diff(c["offsets"].astype(np.int64))
    worst, first_run = {}, None
    for batch_rows in (0, several):
        got = groups.run_grouped(c, batch_rows=batch_rows)
        first_run = first_run or got
        for g in range(G):
            part = groups.group_part(c, got, g)
            assert groups.differing(part, alone[g]) == [], (batch_rows, g)
            if batch_rows:
                continue
            # the sums over the group against the device's own per-record and per-window results, in longdouble
            r0, r1, w0, w1 = spans[g]
            n, R, longest = w1 - w0, r1 - r0, int(lengths[r0:r1].max())
            le = part["L_rec"].astype(LD)
            assert np.array_equal(part["le"], part["L_rec"])
            assert abs(LD(part["L"]) - le.sum()) <= R * U * float(np.abs(le).sum()), g
            post = part["posterior"].astype(LD)
            first = (c["offsets"].astype(np.int64)[r0:r1] - w0)[lengths[r0:r1] > 0]
            nonempty = len(first)
            worst[g] = max(sums_ratio(part["gamma0"], post[first].sum(axis=0), longest, S, R, R, "gamma0 of group %d" % g),
                           sums_ratio(part["Ns"], post.sum(axis=0), longest, S, n, n, "Ns of group %d" % g),
                           sums_ratio(part["T"], post.T @ c["counts"][w0:w1].astype(LD), longest, S, n,
                                      float(c["counts"][w0:w1].sum()), "T of group %d" % g))
            B = cref.posterior_bound(longest, S)
            assert abs(part["xi"].sum() - (n - nonempty)) <= (B + (n + R + 2) * U) * n, g
            assert np.abs(part["posterior"].sum(axis=1) - 1.0).max() <= B + S * U
    statement = check_statement(c, groups.group_part(c, first_run, 1), 1)
    print("fold levels: worst error / bound of the sums per group %s; group 1 against the statement %.3g" % (
        ", ".join("%d: %.3g" % kv for kv in sorted(worst.items())), statement))


# ---- 4: the descriptor tables of one chain under changing masks -----------------------------------------------------------------
def test_the_tables_follow_the_active_mask_on_one_chain():
    from phamers_amd import _lib
    c = groups.group_case(4, 256)
    S, G = c["S"], len(groups.GROUPS) - 1
    rng = np.random.default_rng(5)
    moved = np.exp(c["glogp"] + 0.3 * rng.standard_normal(c["glogp"].shape))
    other = dict(c, glogp=np.log(moved / moved.sum(axis=2, keepdims=True)), gpar=[base.chain_parameters(rng, S, 0.7) for _ in range(G)])
    windows = [s[3] - s[2] for s in gref.group_spans(c["offsets"], c["groups"])]
    largest, small = np.ones(G, dtype=bool), np.ones(G, dtype=bool)
    largest[int(np.argmax(windows))] = False                              # fewer tiles than before
    small[[0, 5]] = False                                                 # two one-window groups: more tiles than before
    assert windows[0] == windows[5] == 1 and int(np.argmax(windows)) == 6
    alone = {id(case): [groups.alone(case, g) for g in range(G)] for case in (c, other)}
    chain = _lib.Chain(_lib.get_context(), c["counts"], c["offsets"], S)
    results = []
    try:
        chain.set_groups(c["groups"])
        for case, active in ((c, None), (c, largest), (c, small), (other, None), (c, None)):
            A, pi, qt, qp = groups.stacked(case)
            chain.set_grouped(case["glogp"], A, pi, qt, qp, case["temper"], active)
            out = dict(E=chain.emissions())
            out["T"], out["Ns"], out["xi"], out["gamma0"], out["L"], out["L_rec"] = chain.expect_grouped(records=True)
            out["state"], out["posterior"], out["le"], out["score"] = chain.decode()
            results.append(out)
            for g in range(G):
                part = groups.group_part(c, out, g)
                if active is None or active[g]:
                    assert groups.differing(part, alone[id(case)][g]) == [], (len(results), g)
                else:
                    assert all(not np.asarray(part[k]).any() for k in groups.OUTPUTS), (len(results), g)
    finally:
        chain.close()
    assert groups.differing(results[0], results[-1]) == []
    assert {"E", "T", "xi", "posterior", "le"} <= set(groups.differing(results[0], results[3]))   # (other parameters, other bits)


# ---- 5: more than one column group in the expectation kernels ----------------------------------------------------------------
def column_rule(Tm, counts, longest, S):
    """|T.sum(axis=0) - col| <= (B + (n + S + 2) u) col, the exact rule of tests/test_gpu_compose.py; the worst ratio."""
    n = len(counts)
    col = counts.sum(axis=0, dtype=np.uint64).astype(np.float64)
    err, bound = np.abs(Tm.sum(axis=0) - col), (cref.posterior_bound(longest, S) + (n + S + 2) * U) * col
    assert (err <= bound).all()
    return float((err[col > 0] / bound[col > 0]).max()) if (col > 0).any() else 0.0


@pytest.mark.parametrize("S", [3, 8])
@pytest.mark.parametrize("D", [320, 16])
def test_more_than_one_column_group(S, D):
    c = groups.group_case(S, D)
    off = c["offsets"].astype(int)
    n, R, longest = len(c["counts"]), len(off) - 1, int(np.diff(off).max())
    A, pi, qt, qp = c["par"]
    got = base.run(c)
    exact = cref.exact_emissions(c["counts"], c["logp"], c["temper"])
    err = np.abs(got["E"].astype(LD) - exact).astype(np.float64)
    bound = cref.emission_bound(c["counts"], c["logp"], c["temper"])
    assert (err <= bound).all()
    states, scores = cref.viterbi_records(got["E"], c["offsets"], qt, qp)
    assert np.array_equal(got["state"], states) and got["score"].tolist() == scores
    want = cref.expect(got["E"], off, A, pi, c["counts"])
    worst = dict(E=float((err / np.maximum(bound, 1e-300)).max()),
                 T=sums_ratio(got["T"], want["T"], longest, S, n, float(c["counts"].sum()), "T"),
                 Ns=sums_ratio(got["Ns"], want["Ns"], longest, S, n, n, "Ns"),
                 columns=column_rule(got["T"], c["counts"], longest, S))
    assert got["T"].shape == (S, D) and (got["T"][:, c["counts"].sum(axis=0) > 0] > 0).all()
    for batch_rows in (1024, 1):
        assert base.same(got, base.run(c, batch_rows=batch_rows)), batch_rows
    grouped = groups.run_grouped(c)
    for batch_rows in (1024, 1):
        assert groups.differing(grouped, groups.run_grouped(c, batch_rows=batch_rows)) == [], batch_rows
    spans = gref.group_spans(c["offsets"], c["groups"])
    for g in range(len(spans)):
        part = groups.group_part(c, grouped, g)
        assert groups.differing(part, groups.alone(c, g)) == [], g
        r0, r1, w0, w1 = spans[g]
        if w1 > w0:
            worst["columns"] = max(worst["columns"], column_rule(part["T"], c["counts"][w0:w1], int(np.diff(off[r0:r1 + 1]).max()), S))
    print("S = %d, D = %d: worst error / bound %s" % (S, D, ", ".join("%s %.3g" % kv for kv in worst.items())))


def test_four_column_groups_from_host_rows_and_a_resident_batch():
    S, D = 3, 1024                                                        # k = 5: four column groups of 256
    c = groups.group_case(S, D)
    off = c["offsets"].astype(int)
    got, grouped = base.run(c), groups.run_grouped(c)
    assert base.same(got, base.run(c, resident=True)) and base.same(got, base.run(c, resident=True, batch_rows=1024))
    assert groups.differing(grouped, groups.run_grouped(c, resident=True)) == []
    assert groups.differing(grouped, groups.run_grouped(c, resident=True, batch_rows=1024)) == []
    worst = column_rule(got["T"], c["counts"], int(np.diff(off).max()), S)
    for g, (r0, r1, w0, w1) in enumerate(gref.group_spans(c["offsets"], c["groups"])):
        assert groups.differing(groups.group_part(c, grouped, g), groups.alone(c, g)) == [], g
        if w1 > w0:
            worst = max(worst, column_rule(grouped["T"][g], c["counts"][w0:w1], int(np.diff(off[r0:r1 + 1]).max()), S))
    print("D = 1024: worst error / bound of the column sums of T %.3g" % worst)


# ---- 6: the row maxima of host emissions past one pass ------------------------------------------------------------------------
def test_row_maxima_past_one_pass():
    S, per = 2, 40
    R = ROWMAX_PASS // per + 6
    n = R * per
    assert ROWMAX_PASS < n - per                                         # the last record lies past the pass
    rng = np.random.default_rng(6)
    offsets = (per * np.arange(R + 1)).astype(np.uint64)
    E = rng.normal(0.0, 2.0, (n, S))
    E[np.arange(n), (np.arange(n) // 11) % S] += 2.0
    case = dict(S=S, par=base.chain_parameters(rng, S, 0.8), temper=1.0, offsets=offsets)
    got = scan.run(case, 0, emissions=E, expect=False)
    lo = R - 200
    part_off = offsets[lo:] - offsets[lo]
    part = scan.run(case, 0, emissions=E[lo * per:], offsets=part_off, expect=False)
    for k in ("state", "posterior"):
        assert np.array_equal(got[k][lo * per:], part[k]), k
    for k in ("le", "score"):
        assert np.array_equal(got[k][lo:], part[k]), k
    states, scores = cref.viterbi_records(E[lo * per:], part_off, case["par"][2], case["par"][3])
    assert np.array_equal(part["state"], states) and part["score"].tolist() == scores
    assert len(set(states.tolist())) == S


# ---- 7: decode without posteriors -----------------------------------------------------------------------------------------------
def test_decode_without_posteriors():
    from phamers_amd import _lib
    ctx = _lib.get_context()
    c = groups.group_case(5, 256, lengths=scan.LENGTHS, groups=[0, 1, 1, 4, 5, 7, 8, 11])
    A, pi, qt, qp = c["par"]
    assert (np.diff(c["offsets"].astype(np.int64)) > T).any()
    for route in ("per record", "scan", "grouped"):
        chain = _lib.Chain(ctx, c["counts"], c["offsets"], c["S"])
        try:
            if route == "grouped":
                chain.set_groups(c["groups"])
                chain.set_grouped(c["glogp"], *groups.stacked(c), c["temper"])
            else:
                chain.set_scan(1 if route == "scan" else 0)
                chain.set(c["logp"], A, pi, qt, qp, c["temper"])
            bare = chain.decode(posterior=False)                          # first: nothing of an earlier decode to find
            state, post, le, score = chain.decode()
            again = chain.decode(posterior=False)
        finally:
            chain.close()
        assert bare[1] is None and again[1] is None and post.shape == (len(c["counts"]), c["S"]), route
        for a, b, d in zip((state, le, score), (bare[0], bare[2], bare[3]), (again[0], again[2], again[3])):
            assert np.array_equal(a, b) and np.array_equal(a, d) and a.any(), route
        assert len(set(state.tolist())) > 1, route
