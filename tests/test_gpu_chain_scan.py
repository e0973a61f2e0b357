"""GPU: the tile scan of the S-state chain (chain.hip) against the per-record route and the
statement of tests/compose_ref.py: the path and its score bit for bit those of the per-record route, posteriors / evidence /
xi / gamma_0 / T / N_s inside the bounds of tests/chain_scan_ref.py of the longdouble statement on the device's own
emissions, a record below the threshold untouched inside a mixed call, a scanned record's bits independent of the call
around it, of the threshold, of batch_rows and of the entry point, more tiles than one launch covers, exact ties at tile
edges, extremes across tile edges, errors, the fit and the command line.  Shapes: records of 1, 2, T - 1, 0, T, T + 1, 2 T,
2 T + 1, 3 T + 5, 1 and 1000 windows in one call (T = phk_chain_tile()), S = 2 .. 8 at D = 256 and S = 3, 4, 8 at D = 30;
more tiles than one launch at every padded width (S = 2, 4, 5).  More scanned records than one carry launch and every tile
count around the carry's look-ahead are tests/test_gpu_chain_shapes.py's."""
import csv
import os

import numpy as np
import pytest

from tests import chain_scan_ref as sref, compose_ref as cref
from tests import test_gpu_compose as base

pytestmark = pytest.mark.gpu
LD = cref.LD
T = sref.TILE
LENGTHS = [1, 2, T - 1, 0, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5, 1, 1000]
KEYS = base.KEYS
PATH = ("state", "score")
ALL = ("E", "T", "Ns", "xi", "gamma0", "L", "L_rec", "state", "posterior", "le", "score")


def run(case, scan=0, batch_rows=0, resident=False, emissions=None, offsets=None, expect=True):
    """dict of everything the device returns for a case (or for host emissions) with records of at least ``scan`` windows on
    the tile scan."""
    from phamers_amd import _lib
    ctx = _lib.get_context()
    A, pi, qt, qp = case["par"]
    off = case["offsets"] if offsets is None else offsets
    batch = _lib.Batch.from_counts(ctx, case["counts"]) if resident else None
    if emissions is not None:
        chain = _lib.Chain(ctx, emissions, off, case["S"], emissions=True)
    else:
        chain = _lib.Chain(ctx, batch if resident else case["counts"], off, case["S"], batch_rows)
    try:
        chain.set_scan(scan)
        chain.set(None if emissions is not None else case["logp"], A, pi, qt, qp, case["temper"])
        out = dict(E=chain.emissions() if emissions is None else np.asarray(emissions))
        if expect:
            out["T"], out["Ns"], out["xi"], out["gamma0"], out["L"], out["L_rec"] = chain.expect(records=True)
        out["state"], out["posterior"], out["le"], out["score"] = chain.decode()
    finally:
        chain.close()
        if batch is not None:
            batch.close()
    return out


def record_equal(a, b, off_a, ra, off_b, rb, keys=("E", "state", "posterior")):
    sa, sb = slice(int(off_a[ra]), int(off_a[ra + 1])), slice(int(off_b[rb]), int(off_b[rb + 1]))
    return (all(np.array_equal(a[k][sa], b[k][sb]) for k in keys) and a["le"][ra] == b["le"][rb]
            and a["score"][ra] == b["score"][rb])


@pytest.fixture(scope="module")
def tile():
    from phamers_amd import _lib
    assert int(_lib.load().phk_chain_tile()) == T
    return T


@pytest.fixture(scope="module")
def cases(tile):
    out = {key: base.make_case(key[0], key[1], seed=3, lengths=LENGTHS) for key in KEYS}
    for c in out.values():
        c["off"] = run(c, 0)
        c["on"] = run(c, 1)
    return out


@pytest.mark.parametrize("key", KEYS)
def test_path_and_score_are_those_of_the_per_record_route(cases, key):
    c = cases[key]
    assert np.array_equal(c["on"]["E"], c["off"]["E"])
    assert np.array_equal(c["on"]["state"], c["off"]["state"]) and np.array_equal(c["on"]["score"], c["off"]["score"])
    A, pi, qt, qp = c["par"]
    states, scores = cref.viterbi_records(c["on"]["E"], c["offsets"], qt, qp)
    assert np.array_equal(c["on"]["state"], states) and c["on"]["score"].tolist() == scores
    assert len(set(states.tolist())) > 1                                  # the path changes state


@pytest.mark.parametrize("key", KEYS)
def test_expectations_within_the_scan_bounds(cases, key):
    c, got = cases[key], cases[key]["on"]
    S, off = c["S"], c["offsets"].astype(int)
    A, pi = c["par"][:2]
    n, R, longest = len(c["counts"]), len(off) - 1, int(np.diff(off).max())
    want = cref.expect(got["E"], off, A, pi, c["counts"])
    worst = {}
    worst["posterior"] = max(sref.check_posterior(got["posterior"][off[r]:off[r + 1]], want["gamma"][off[r]:off[r + 1]],
                                                  off[r + 1] - off[r], S, "posterior of record %d" % r) for r in range(R))
    M = got["E"].max(axis=1)
    worst["evidence"] = max(sref.check_evidence(got["le"][r], want["log_evidence_rec"][r], M[off[r]:off[r + 1]], S,
                                                "record %d" % r) for r in range(R))
    assert np.array_equal(got["le"], got["L_rec"])                      # decode and expect: the same passes
    total = sum(sref.scan_evidence_bound(M[off[r]:off[r + 1]], S, want["log_evidence_rec"][r]) for r in range(R))
    total += R * cref.U * float(np.abs(want["log_evidence_rec"]).sum())
    assert abs(LD(got["L"]) - want["log_evidence"]) <= total
    worst["xi"] = sref.check_sums(got["xi"], want["xi"], longest, S, n + R, n, "xi")
    worst["gamma0"] = sref.check_sums(got["gamma0"], want["gamma0"], longest, S, R, R, "gamma0")
    worst["T"] = sref.check_sums(got["T"], want["T"], longest, S, n, float(c["counts"].sum()), "T")
    worst["Ns"] = sref.check_sums(got["Ns"], want["Ns"], longest, S, n, n, "Ns")
    print("scan %r: worst error / bound %s" % (key, ", ".join("%s %.3g" % kv for kv in worst.items())))
    B = sref.scan_posterior_bound(longest, S)
    assert np.abs(got["posterior"].sum(axis=1) - 1.0).max() <= B + S * cref.U


@pytest.mark.parametrize("key", [(2, 256), (5, 256), (8, 30)])
def test_mixed_call(cases, key):
    c = cases[key]
    off = c["offsets"].astype(int)
    mixed = run(c, T + 1)
    for r in range(len(off) - 1):
        other = c["off"] if off[r + 1] - off[r] <= T else c["on"]
        assert record_equal(mixed, other, off, r, off, r), r
    short = np.diff(off) <= T
    assert short.any() and not short.all()
    assert base.same(mixed, run(c, T + 1), ALL)                           # two runs are identical, the sums over the records too


@pytest.mark.parametrize("S", [3, 8])
def test_a_scanned_record_alone_gives_the_bits_it_gives_inside_a_shuffled_call(cases, S):
    c = cases[(S, 256)]
    got, off = c["on"], c["offsets"].astype(int)
    order = np.random.default_rng(S).permutation(len(off) - 1)
    rows = np.concatenate([np.arange(off[r], off[r + 1]) for r in order]).astype(int)
    shuffled = dict(c, counts=c["counts"][rows], offsets=np.concatenate(([0], np.cumsum(np.diff(off)[order]))).astype(np.uint64))
    sh = run(shuffled, 1)
    at = shuffled["offsets"].astype(int)
    for i, r in enumerate(order):
        assert record_equal(got, sh, off, r, at, i), r
    for r in (2, 5, 8, 10):                                               # T - 1, T + 1, 3 T + 5 and 1000 windows, alone
        a, b = off[r], off[r + 1]
        alone = run(dict(c, counts=c["counts"][a:b], offsets=np.array([0, b - a], dtype=np.uint64)), b - a)
        assert record_equal(got, alone, off, r, [0, b - a], 0), r


@pytest.mark.parametrize("S", [2, 5])
def test_same_bits_from_host_rows_a_resident_batch_and_any_batch_rows(cases, S):
    c = cases[(S, 256)]
    assert len(c["counts"]) > 1025
    for kw in (dict(batch_rows=1), dict(batch_rows=1025), dict(resident=True), dict(resident=True, batch_rows=1025)):
        assert base.same(c["on"], run(c, 1, **kw), ALL), kw
    # host emissions: the chain half, on the device's own E
    em = run(c, 1, emissions=c["on"]["E"])
    for k in ("xi", "gamma0", "L", "L_rec", "state", "posterior", "le", "score"):
        assert np.array_equal(em[k], c["on"][k]), k


@pytest.mark.parametrize("S", [2, 4, 5])
def test_more_tiles_than_one_launch_covers(S):
    from phamers_amd import _lib
    n_long = int(_lib.load().phk_chain_scan_grid_pass()) * T + 3 * T + 1
    rng = np.random.default_rng(S)
    lengths = [3, T + 2, n_long, 0, 2 * T, 5]
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
    n = int(offsets[-1])
    favoured = (np.arange(n) // 37) % S
    E = rng.normal(0.0, 1.5, (n, S))
    E[np.arange(n), favoured] += 2.0
    case = dict(S=S, par=base.chain_parameters(rng, S, 0.9), temper=1.0, offsets=offsets)
    seq = run(case, 0, emissions=E, expect=False)
    got = run(case, 1, emissions=E, expect=False)
    assert np.array_equal(got["state"], seq["state"]) and np.array_equal(got["score"], seq["score"])
    off = offsets.astype(int)
    worst = 0.0
    for r, length in enumerate(lengths):
        a, b = off[r], off[r + 1]
        extra = cref.posterior_bound(length, S)                           # the per-record route's own distance from the exact value
        worst = max(worst, sref.check_posterior(got["posterior"][a:b], seq["posterior"][a:b].astype(LD), length, S,
                                                "record %d" % r, extra=extra))
        M = E[a:b].max(axis=1)
        both = sref.scan_evidence_bound(M, S, seq["le"][r]) + cref.evidence_bound(M, S, seq["le"][r])
        assert abs(LD(got["le"][r]) - LD(seq["le"][r])) <= both, r
    print("S = %d, %d tiles: worst distance from the per-record route / (B + B_scan) %.3g" % (S, n_long // T + 1, worst))
    mixed = run(case, n_long, emissions=E, expect=False)                    # only the long record on the scan
    for r in range(len(lengths)):
        assert record_equal(mixed, got if r == 2 else seq, off, r, off, r), r


def test_exact_ties_across_tiles():
    S, n = 3, 3 * T + 5
    offsets = np.array([0, n], dtype=np.uint64)
    A, pi = np.full((S, S), 1.0 / 3.0), np.full(S, 1.0 / 3.0)              # (three thirds add to 1 exactly)
    par = (A, pi, cref.quantise_log(A), cref.quantise_log(pi))
    case = dict(S=S, par=par, temper=1.0, offsets=offsets)
    got = run(case, 1, emissions=np.full((n, S), -2.5))
    assert (got["state"] == 0).all() and np.abs(got["posterior"] - 1.0 / 3.0).max() <= sref.scan_posterior_bound(n, S)
    # states 1 and 2 equal and better than 0 at a tile's last and first step; a later tile's first step prefers 2
    E = np.zeros((n, S))
    E[T - 1], E[T], E[2 * T] = [-5.0, 0.0, 0.0], [-5.0, 0.0, 0.0], [-5.0, -1.0, 0.0]
    got = run(case, 1, emissions=E)
    states, scores = cref.viterbi_records(E, offsets, par[2], par[3])
    assert np.array_equal(got["state"], states) and got["score"].tolist() == scores
    assert np.array_equal(got["state"], run(case, 0, emissions=E)["state"])
    assert got["state"][T - 1] == got["state"][T] == 1 and got["state"][2 * T] == 2


@pytest.mark.parametrize("S", [2, 5])
def test_extremes_across_tile_edges(S):
    rng = np.random.default_rng(70 + S)
    n = 3 * T + 5
    offsets = np.array([0, n], dtype=np.uint64)
    A = np.full((S, S), 1e-12)
    np.fill_diagonal(A, 1.0 - (S - 1) * 1e-12)
    pi = np.full(S, 1.0 / S)
    pi[0] = 1.0 - pi[1:].sum()
    case = dict(S=S, par=(A, pi, cref.quantise_log(A), cref.quantise_log(pi)), temper=1.0, offsets=offsets)
    # emission gaps of 1e5 nats (exp underflows, the integers are clamped at -2^15), the favoured state changing every 9 windows
    # and at both sides of every tile edge
    E = np.full((n, S), -1e5) * (0.5 + 0.5 * rng.random((n, S)))
    favoured = (np.arange(n) // 9) % S
    for edge in range(T, n, T):
        favoured[edge:] = (favoured[edge:] + (favoured[edge] == favoured[edge - 1])) % S
    E[np.arange(n), favoured] = 0.0
    # a run of windows without k-mers (E = 0 in every state) across the second tile edge
    E[2 * T - 4:2 * T + 5] = 0.0
    got, seq = run(case, 1, emissions=E), run(case, 0, emissions=E)
    for k in ("posterior", "le", "xi", "gamma0", "L"):
        assert np.isfinite(got[k]).all(), k
    want = cref.expect(E, offsets, A, pi)
    worst = sref.check_posterior(got["posterior"], want["gamma"], n, S, "extremes")
    sref.check_sums(got["xi"], want["xi"], n, S, n + 1, n, "xi")
    sref.check_evidence(got["le"][0], want["log_evidence_rec"][0], E.max(axis=1), S, "extremes")
    print("extremes S = %d: worst error / bound %.3g" % (S, worst))
    assert np.array_equal(got["state"], seq["state"]) and np.array_equal(got["score"], seq["score"])
    states, scores = cref.viterbi_records(E, offsets, case["par"][2], case["par"][3])
    assert np.array_equal(got["state"], states) and got["score"].tolist() == scores


def test_errors_and_switching_the_route_off_again(cases):
    from phamers_amd import _lib
    ctx, lib = _lib.get_context(), _lib.load()
    c = cases[(3, 256)]
    A, pi, qt, qp = c["par"]
    assert lib.phk_chain_set_scan(ctx.handle, None, 1) == _lib.PHK_ERR_ARG
    assert "NULL chain" in _lib.last_error()
    chain = _lib.Chain(ctx, c["counts"], c["offsets"], 3)
    try:
        with pytest.raises(ValueError):
            chain.set_scan(-1)
        chain.set_scan(1)                                                # before the set
        chain.set(c["logp"], A, pi, qt, qp, c["temper"])
        on = chain.decode()
        chain.set_scan(10 ** 9)                                          # no record reaches it
        none = chain.decode()
        chain.set_scan(1)                                                # after the set
        again = chain.decode()
        xi_on = chain.expect()[2]
        chain.set_scan(0)
        off = chain.decode()
        xi_off = chain.expect()[2]
    finally:
        chain.close()
    for got, want in ((on, c["on"]), (again, c["on"]), (none, c["off"]), (off, c["off"])):
        assert np.array_equal(got[0], want["state"]) and np.array_equal(got[1], want["posterior"])
        assert np.array_equal(got[2], want["le"]) and np.array_equal(got[3], want["score"])
    assert np.array_equal(xi_on, c["on"]["xi"]) and np.array_equal(xi_off, c["off"]["xi"])
    # nothing to do is no error
    empty = _lib.Chain(ctx, np.zeros((0, 256), dtype=np.uint32), [0, 0, 0], 3)
    empty.set_scan(1)
    empty.set(c["logp"], A, pi, qt, qp, 1.0)
    assert not empty.expect()[2].any() and len(empty.decode()[0]) == 0
    empty.close()


# ---- the fit and the command line on the "small" sequence ---------------------------------------------------------------------
def test_fit_and_decode_on_the_small_sequence(tile):
    from phamers_amd import compose
    C = cref.window_counts(cref.small_sequence(2))
    off = [0, len(C)]
    comp = compose.fit(C, off, 3, scan=1)
    assert comp.converged
    dec = comp.decode(C, off, scan=1)
    assert cref.changes(dec.state) == [12000, 20000, 30000] and dec.state[0] == dec.state[-1]
    plain = comp.decode(C, off)
    assert np.array_equal(plain.state, dec.state) and np.array_equal(plain.path_score_q, dec.path_score_q)
    assert np.abs(plain.posterior - dec.posterior).max() <= 2 * sref.scan_posterior_bound(len(C), 3)
    # True: no record of this sequence reaches SCAN_FROM, so the bits are those of the route off
    assert len(C) < compose.SCAN_FROM
    same = comp.decode(C, off, scan=True)
    assert np.array_equal(same.posterior, plain.posterior) and np.array_equal(same.log_evidence, plain.log_evidence)


def test_command_line_with_scan(tmp_path):
    from phamers_amd import compose
    seq = cref.small_sequence(2)
    fasta = str(tmp_path / "genome.fasta")
    with open(fasta, "w") as f:
        f.write(">genome\n" + "\n".join(seq[i:i + 80] for i in range(0, len(seq), 80)) + "\n")
    segments = {}
    for name, extra in (("off", []), ("on", ["--scan", "1"])):
        out = str(tmp_path / name)
        result = compose.main(["-in", fasta, "-out", out, "-S", "3"] + extra)
        assert len(result) == 80
        for file in ("compose_windows.csv", "compose_segments.csv", "compose_profiles.csv", "compose_trace.csv"):
            assert os.path.getsize(os.path.join(out, file)) > 0, file
        rows = list(csv.DictReader(open(os.path.join(out, "compose_segments.csv"))))
        segments[name] = [(r["record_id"], int(r["start"]), int(r["end"]), r["state"], int(r["n_windows"])) for r in rows]
    assert [s[2] for s in segments["on"]] == [12000, 20000, 30000, 40000]
    assert segments["on"] == segments["off"]
