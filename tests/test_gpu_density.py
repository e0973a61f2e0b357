"""GPU: the density scoring method (Gaussian kernel density log-likelihood ratio, density.hip) against the reference's
scikit-learn result (tests/golden/scoring_density.npz, tools/gen_golden_density.py) and against a dense float64
restatement (tests/density_ref.py).  Bars: 1e-9 x max(1, |want|) against scikit-learn (its tree is off by up to ~1e-9
itself), 1e-11 x max(1, |want|) against the restatement, bit equality across batch splits and entry points."""

import numpy as np
import pytest

from tests import density_ref, helpers

pytestmark = pytest.mark.gpu
SKL = 1e-9
F64 = 1e-11


def _ref_matrices():
    from oracle import oracle
    ref = helpers.load_npz("ref_features.npz")
    pos = oracle.normalize_counts(ref["pos_counts"].astype(np.int64))
    neg = oracle.normalize_counts(ref["neg_counts"].astype(np.int64))
    return pos, neg


def _queries(g):
    return np.vstack((helpers.load_npz("scoring_k4.npz")["q"], g["adv_q"]))


@pytest.mark.parametrize("tag", ["full", "eq"])
def test_score_points_density_matches_reference(tag):
    from phamers_amd import phamer
    g = helpers.load_npz("scoring_density.npz")
    pos, neg = _ref_matrices()
    q = _queries(g)
    if tag == "eq":
        m = int(g["n_equalized"][0])
        pos, neg = pos[:m], neg[:m]
    got = phamer.score_points(q, pos, neg, method="density")
    assert density_ref.close(got, g["density_" + tag], SKL)
    assert density_ref.close(got, density_ref.density_scores(q, pos, neg), F64)
    sc = phamer.phamer_scorer()
    sc.scoring_method = "density"
    sc.data_points, sc.positive_data, sc.negative_data = q, pos, neg
    assert np.array_equal(sc.score_points(), got)
    assert sc.positive_centroids is None and sc.negative_centroids is None   # no k-means fit for density


def test_bandwidths_and_get_density():
    from phamers_amd import learning, phamer
    g = helpers.load_npz("scoring_density.npz")
    pos, neg = _ref_matrices()
    q = helpers.load_npz("scoring_k4.npz")["q"]
    for i, (hp, hn) in enumerate(g["bandwidth_pairs"]):
        sc = phamer.phamer_scorer()
        sc.scoring_method = "density"
        sc.positive_bandwidth, sc.negative_bandwidth = float(hp), float(hn)
        sc.data_points, sc.positive_data, sc.negative_data = q, pos, neg
        got = sc.score_points()
        assert density_ref.close(got, g["density_full_bw%d" % i], SKL)
        assert density_ref.close(got, density_ref.density_scores(q, pos, neg, hp, hn), F64)
    pts = np.vstack((q[:10], g["adv_q"]))
    gp = np.array([learning.get_density(p, pos) for p in pts])
    gn = np.array([learning.get_density(p, neg) for p in pts])
    assert isinstance(learning.get_density(pts[0], pos), float)
    assert density_ref.close(gp, g["get_density_pos"], SKL) and density_ref.close(gn, g["get_density_neg"], SKL)
    assert np.array_equal(learning.log_density(pts, pos, 0.1), gp)
    assert density_ref.close(gp, density_ref.log_density(pts, pos, 0.1), F64)


def test_far_query_does_not_underflow():
    """The homopolymer profile lies at d^2 ~ 1 from every row: exponents ~ -2e4, a plain sum of exp would be 0."""
    from phamers_amd import phamer
    g = helpers.load_npz("scoring_density.npz")
    pos, neg = _ref_matrices()
    homo = g["adv_q"][:1]
    assert homo[0, 0] == 1.0 and homo[0, 1:].sum() == 0.0
    got = phamer.score_points(homo, pos, neg, method="density")
    n = helpers.load_npz("scoring_k4.npz")["q"].shape[0]
    assert np.all(np.isfinite(got))
    assert density_ref.close(got, g["density_full"][n:n + 1], SKL)
    assert density_ref.close(got, density_ref.density_scores(homo, pos, neg), F64)


@pytest.mark.parametrize("k", [5, 6])
def test_high_dimensional_sets(k):
    from phamers_amd import phamer
    g = helpers.load_npz("scoring_density.npz")
    h = helpers.load_npz("scoring_highdim.npz")
    t = "k%d" % k
    q, pos, neg = h["q_" + t], h["pos_" + t], h["neg_" + t]
    got = phamer.score_points(q, pos, neg, method="density")
    assert density_ref.close(got, g["density_" + t], SKL)
    assert density_ref.close(got, density_ref.density_scores(q, pos, neg), F64)


def test_shapes():
    """M not a multiple of any tile, the class boundary inside a 16-row block, N in {0, 1, 17, 4097}; an odd D through the
    standalone entry."""
    from phamers_amd import _lib, learning
    pos, neg = _ref_matrices()
    p, n = pos[:301], neg[:77]
    ctx = _lib.get_context()
    model = _lib.Model(ctx, p, n, k_neighbors=3)
    rng = np.random.default_rng(3)
    Q = np.vstack((pos, neg))[rng.choice(pos.shape[0] + neg.shape[0], 4097, replace=False)]
    want = density_ref.density_scores(Q, p, n)
    for N in (0, 1, 17, 4097):
        got = model.score(Q[:N], "density")
        assert got.shape == (N,)
        assert density_ref.close(got, want[:N], F64)
    model.close()
    X = rng.random((37, 33))
    X /= X.sum(axis=1, keepdims=True)
    Qo = rng.random((19, 33))
    Qo /= Qo.sum(axis=1, keepdims=True)
    assert density_ref.close(learning.log_density(Qo, X, 0.05), density_ref.log_density(Qo, X, 0.05), F64)


def test_nan_rows_and_bad_bandwidths():
    from phamers_amd import _lib, learning, phamer
    pos, neg = _ref_matrices()
    q = helpers.load_npz("scoring_k4.npz")["q"][:20].copy()
    q[4] = np.nan
    with pytest.raises(ValueError):
        phamer.score_points(q, pos, neg, method="density")
    with pytest.raises(ValueError):   # a contig shorter than k: a zero-count row on the device
        phamer.score_contigs(["ACGTACGTAAC" * 500, "ACG"], pos, neg, method="density")
    ctx = _lib.get_context()
    model = _lib.Model(ctx, pos[:100], neg[:100], k_neighbors=3)
    for bad in (0.0, -0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            model.set_bandwidths(bad, 0.01)
        with pytest.raises(ValueError):
            model.set_bandwidths(0.005, bad)
        assert ctx.lib.phk_model_set_bandwidths(ctx.handle, model.handle, bad, 0.01) == _lib.PHK_ERR_ARG
        assert ctx.lib.phk_kde_log_density(ctx.handle, _lib.ptr(q[:2]), 2, _lib.ptr(pos[:10]), 10, 256, bad,
                                           _lib.ptr(np.empty(2))) == _lib.PHK_ERR_ARG
        with pytest.raises(ValueError):
            learning.get_density(q[0], pos, bandwidth=bad)
        sc = phamer.phamer_scorer()
        sc.scoring_method = "density"
        sc.positive_bandwidth = bad
        sc.data_points, sc.positive_data, sc.negative_data = q[:3], pos, neg
        with pytest.raises(ValueError):
            sc.score_points()
    # the model kept its last good bandwidths
    assert density_ref.close(model.score(q[:3], "density"), density_ref.density_scores(q[:3], pos[:100], neg[:100]), F64)
    # density cannot be OR-ed with the other methods
    out = np.empty(3)
    for m in (5, 6, 7):
        assert ctx.lib.phk_score(ctx.handle, model.handle, _lib.ptr(q[:3]), 3, m, _lib.ptr(out)) == _lib.PHK_ERR_ARG
    # a class without unmasked rows is refused
    mask = np.zeros(200, np.uint8)
    mask[:100] = 1
    model.set_column_mask(mask)
    with pytest.raises(_lib.PhkError):
        model.score(q[:3], "density")
    model.close()


def test_resident_batch_entry_points_and_splits():
    """Host rows, resident counts (Batch.score), phk_score_counts_dev, phk_count_score_dev: bit for bit; so are the batch
    splits 1/2/4/8."""
    from oracle import oracle
    from phamers_amd import _lib, device, synth
    pos, neg = _ref_matrices()
    ctx = _lib.get_context()
    model = _lib.Model(ctx, pos, neg, k_neighbors=3)
    n, L = 1000, 5000
    seqs = synth.synth_contigs(4, n, L)
    rows = oracle.normalize_counts(oracle.count(seqs, 4))
    host = model.score(rows, "density")
    assert density_ref.close(host, density_ref.density_scores(rows, pos, neg), F64)
    batch = _lib.Batch.from_sequences(ctx, list(seqs), 4)
    assert np.array_equal(batch.score(model, "density"), host)
    batch.close()
    T = n * L
    d_packed = device.DeviceArray(ctx, device.packed_words(T), np.uint32)
    d_off = device.DeviceArray(ctx, n + 1, np.uint64)
    device.synth_packed(ctx, 4, 0, n, L, d_packed, d_off)
    d_counts = device.DeviceArray(ctx, (n, 256), np.uint32)
    d_scores = device.DeviceArray(ctx, n, np.float64)
    d_status = device.DeviceArray.from_host(ctx, np.zeros(1, np.uint32))
    device.count_score(ctx, model, d_packed, None, T, d_off, n, 4, "density", d_counts, d_scores, d_status)
    ctx.sync()
    assert d_status.to_host()[0] == 0
    assert np.array_equal(d_scores.to_host(), host)
    for parts in (1, 2, 4, 8):
        d_part = device.DeviceArray(ctx, n, np.float64)
        cuts = np.linspace(0, n, parts + 1).astype(np.int64)
        for a, b in zip(cuts[:-1], cuts[1:]):
            device.score_counts(ctx, model, d_counts.ptr + int(a) * 256 * 4, int(b - a), "density", d_part.ptr + int(a) * 8)
        assert np.array_equal(d_part.to_host(), host), parts
        d_Q = device.DeviceArray.from_host(ctx, rows)
        device.score(ctx, model, d_Q.ptr + int(cuts[1]) * 256 * 8, n - int(cuts[1]), "density", d_part.ptr)
        assert np.array_equal(d_part.to_host()[:n - int(cuts[1])], host[int(cuts[1]):]), parts
    # force_exact / proposal knobs do not touch density
    with ctx.options(force_exact=("1", "0")):
        assert np.array_equal(model.score(rows, "density"), host)
    model.close()


def test_cross_validation_density():
    """cross_validator(method='density') on the resident model against the reference's seeded run; every fold equals a model
    built from the fold's training rows alone (the mask takes the held-out rows out of the sums AND out of n_c_eff)."""
    from phamers_amd import _lib, cross_validate
    g = helpers.load_npz("scoring_density.npz")
    pos, neg = _ref_matrices()
    seed, N, n_p, n_n = (int(x) for x in g["cv_meta"])
    v = cross_validate.cross_validator()
    v.positive_data, v.negative_data = pos, neg
    v.equalize_reference = True
    v.N = N
    v.method = "density"
    v.seed = seed
    ps, ns = v.cross_validate()
    assert v.model_uploads == 1
    assert np.array_equal(v.positive_assignment, g["cv_pos_asmt"]) and np.array_equal(v.negative_assignment, g["cv_neg_asmt"])
    # the reference's run wherever scikit-learn's KD tree and a ball tree agree to 1e-10 (tools/gen_golden_density.py: on a few
    # held-out rows its tree sums are off, by up to ~10 nats); every row, the disputed ones included, against a model built
    # from the fold's training rows alone below
    for got, c in ((ps, "pos"), (ns, "neg")):
        ref, ball = g["cv_%s_scores" % c], g["cv_%s_scores_balltree" % c]
        ok = np.abs(ref - ball) <= 1e-10 * np.maximum(1.0, np.abs(ball))
        assert ok.mean() >= 0.97
        assert density_ref.close(got[ok], ref[ok], SKL)
    P, Nm = pos[:n_p], neg[:n_n]
    ctx = _lib.get_context()
    for fold in range(N):
        out_p, out_n = v.positive_assignment == fold, v.negative_assignment == fold
        alone = _lib.Model(ctx, P[~out_p], Nm[~out_n], k_neighbors=3)
        want = alone.score(np.vstack((P[out_p], Nm[out_n])), "density")
        alone.close()
        got = np.concatenate((ps[out_p], ns[out_n]))
        assert density_ref.close(got, want, F64), fold


def test_two_pow_20_synthetic_contigs():
    """2^20 resident 5 kb contigs against the real reference, count -> density: 4096 sampled rows against the float64
    restatement, and the split invariance of the whole batch."""
    from oracle import oracle
    from phamers_amd import _lib, device
    pos, neg = _ref_matrices()
    ctx = _lib.get_context()
    model = _lib.Model(ctx, pos, neg, k_neighbors=3)
    n, L = 1 << 20, 5000
    T = n * L
    d_packed = device.DeviceArray(ctx, device.packed_words(T), np.uint32)
    d_off = device.DeviceArray(ctx, n + 1, np.uint64)
    device.synth_packed(ctx, 0, 0, n, L, d_packed, d_off)
    d_counts = device.DeviceArray(ctx, (n, 256), np.uint32)
    d_scores = device.DeviceArray(ctx, n, np.float64)
    d_status = device.DeviceArray.from_host(ctx, np.zeros(1, np.uint32))
    device.count_score(ctx, model, d_packed, None, T, d_off, n, 4, "density", d_counts, d_scores, d_status)
    ctx.sync()
    assert d_status.to_host()[0] == 0
    full = d_scores.to_host()
    assert np.all(np.isfinite(full))
    rng = np.random.default_rng(0)
    sample = np.sort(rng.choice(n, 4096, replace=False))
    rows = oracle.normalize_counts(device.read_rows(ctx, d_counts, sample, 256).astype(np.int64))
    assert density_ref.close(full[sample], density_ref.density_scores(rows, pos, neg), F64)
    d_part = device.DeviceArray(ctx, n, np.float64)
    for parts in (2, 8):
        cuts = np.linspace(0, n, parts + 1).astype(np.int64)
        for a, b in zip(cuts[:-1], cuts[1:]):
            device.score_counts(ctx, model, d_counts.ptr + int(a) * 256 * 4, int(b - a), "density", d_part.ptr + int(a) * 8)
        assert np.array_equal(d_part.to_host(), full), parts
    model.close()


def _profiled(ctx, fn):
    """fn() with the profiler on: (its result, {kernel: launches})."""
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        out = fn()
        return out, {k: v[1] for k, v in ctx.profile().items()}
    finally:
        ctx.profile_enable(False)


@pytest.mark.parametrize("D", [1, 31, 33, 65])
def test_odd_widths_across_chunks_and_query_blocks(D):
    """The fp64 Gram tile with D % 32 != 0 (phk_kde_partial_kernel<false>) for M around the 256-row chunk and N around the
    128-query block: within F64 of the restatement, and bit-identical whatever the split of the queries across calls."""
    from phamers_amd import learning
    rng = np.random.default_rng(D)
    h = 0.25 * np.sqrt(D)
    for M in (1, 255, 256, 257, 513):
        X = rng.random((M, D))
        Q = np.vstack((X[rng.integers(0, M, 2048)] + rng.normal(size=(2048, D)) * 0.1, rng.random((2049, D)) * 1.5))
        want = density_ref.log_density(Q, X, h)
        full = learning.log_density(Q, X, h)
        assert density_ref.close(full, want, F64), M
        for N in (1, 127, 128, 129, 4097):
            got = learning.log_density(Q[:N], X, h)
            assert np.array_equal(got, full[:N]), (M, N)
        parts = [learning.log_density(Q[a:b], X, h) for a, b in ((0, 129), (129, 2049), (2049, 4097))]
        assert np.array_equal(np.concatenate(parts), full), M


def test_query_batches_at_4096_columns():
    """D = 4096 caps a launch at 8 192 queries (256 MiB of queries): 8 300 queries run in two batches, within F64 of the
    restatement and bit-identical to the queries scored in one call each side of the cut."""
    from phamers_amd import _lib, learning
    rng = np.random.default_rng(4096)
    D, M, N = 4096, 300, 8300
    X = rng.random((M, D))
    Q = np.vstack((X[rng.integers(0, M, N // 2)] + rng.normal(size=(N // 2, D)) * 0.01, rng.random((N - N // 2, D))))
    h = 4.0
    got, launches = _profiled(_lib.get_context(), lambda: learning.log_density(Q, X, h))
    assert launches.get("phk_kde_merge_kernel", 0) >= 2, launches
    assert density_ref.close(got, density_ref.log_density(Q, X, h), F64)
    for a, b in ((0, 8191), (8191, 8193), (8193, N)):
        assert np.array_equal(learning.log_density(Q[a:b], X, h), got[a:b]), (a, b)
