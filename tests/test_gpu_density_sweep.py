"""GPU: the density bandwidth sweep (density_sweep.hip, learning.density_sweep) and the bandwidth grid on top of it
(phamers_amd/bandwidth.py).  The contract: row b of a sweep is bit for bit ``learning.log_density`` at bandwidth b, for any
number of bandwidths, pass split and query batch; the leave-one-out rows meet the dense restatement
(tests/density_sweep_ref.py) at the bar of tests/test_gpu_density.py, 1e-11 x max(1, |want|).

Shapes: 300 data rows (chunks of 256 + 44) and 130 queries (query blocks of 128 + 2 for the batch loop and the kernel of
passes of one or two bandwidths, 64 + 64 + 2 for the kernel of wider passes)."""
import numpy as np
import pytest

from tests import density_ref, density_sweep_ref, helpers

pytestmark = pytest.mark.gpu
F64 = 1e-11


def _rows(n, D, seed):
    """Normalised rows (non-negative, row sum 1) a few hundredths apart, like normalised k-mer counts."""
    rng = np.random.default_rng(seed)
    base = rng.random(D) + 0.5
    x = base[None, :] * (1.0 + 0.3 * rng.standard_normal((n, D))).clip(0.05)
    return x / x.sum(axis=1, keepdims=True)


def _per_pass():
    from phamers_amd import learning
    return learning.DENSITY_SWEEP_PER_PASS


def _bandwidths(B):
    """Unsorted, with a repeated value wherever B >= 3."""
    pool = [0.02, 0.004, 0.05, 0.004, 0.3, 0.0025, 0.01, 0.1, 0.007, 0.03, 0.002, 0.2]
    return [pool[i % len(pool)] for i in range(B)]


@pytest.mark.parametrize("D", [7, 32, 256])
def test_bit_equal_to_log_density_per_bandwidth(D):
    from phamers_amd import learning
    NB = _per_pass()
    X, Q = _rows(300, D, 1), _rows(130, D, 2)
    singles = {}
    for B in (1, 2, 3, NB, NB + 1):      # 2 | 3: where a pass changes from the wide-tile kernel to the narrow one
        hs = _bandwidths(B)
        for h in hs:
            if h not in singles:
                singles[h] = learning.log_density(Q, X, h)
        got = learning.density_sweep(Q, X, hs)
        assert got.shape == (B, 130) and got.dtype == np.float64
        for b, h in enumerate(hs):
            assert np.array_equal(got[b], singles[h]), (D, B, b, h)
        if B >= 4:
            assert hs[1] == hs[3] and np.array_equal(got[1], got[3])
        assert np.array_equal(learning.density_sweep(Q, X, hs, _per_pass=1), got)
        assert np.array_equal(learning.density_sweep(Q, X, hs, _batch_rows=128), got)
    h0 = _bandwidths(1)[0]
    assert density_ref.close(singles[h0], density_ref.log_density(Q, X, h0), F64)


def test_far_apart_bandwidths_share_one_pass():
    """h = 0.002 and h = 0.5 in one pass; the homopolymer profile lies at d^2 ~ 1 from every row: exponents ~ -1.25e5
    at the narrow bandwidth and ~ -2 at the wide one, so one shift for both would flush the narrow sums to 0."""
    from phamers_amd import learning
    assert _per_pass() >= 2
    X, Q = _rows(300, 256, 3), _rows(130, 256, 4)
    Q[5] = 0.0
    Q[5, 0] = 1.0
    hs = [0.002, 0.5]
    got = learning.density_sweep(Q, X, hs)
    assert np.all(np.isfinite(got))
    d2 = ((Q[5][None, :] - X) ** 2).sum(axis=1)
    assert 0.9 < d2.min() and (-d2.min() / (2 * 0.002 ** 2)) < -1.1e5
    for b, h in enumerate(hs):
        assert np.array_equal(got[b], learning.log_density(Q, X, h))
        assert density_ref.close(got[b], density_ref.log_density(Q, X, h), F64)


def _exclude_cases():
    dup = _rows(300, 32, 8)
    dup[200] = dup[3]
    return {"M300": _rows(300, 256, 5), "M257": _rows(257, 32, 6), "M2": _rows(2, 32, 7), "dup": dup}


@pytest.mark.parametrize("case", ["M300", "M257", "M2", "dup"])
def test_exclude_self(case):
    from phamers_amd import learning
    NB = _per_pass()
    X = _exclude_cases()[case]
    hs = [0.01, 0.003, 0.05]
    want = density_sweep_ref.log_density_sweep(X, X, hs, exclude_self=True)
    got = learning.density_sweep(X, X, hs, exclude_self=True)
    assert got.shape == want.shape
    assert density_ref.close(got, want, F64)
    for per in (1, NB):
        for rows in (0, 128):
            assert np.array_equal(learning.density_sweep(X, X, hs, exclude_self=True, _per_pass=per, _batch_rows=rows), got)
    M, D = X.shape
    if case == "M2":    # one surviving term: L = -d^2 / 2 h^2 - lognorm
        d2 = ((X[0] - X[1]) ** 2).sum()
        for b, h in enumerate(hs):
            lone = -d2 / (2 * h * h) - (np.log(1.0) + 0.5 * D * np.log(2 * np.pi) + D * np.log(h))
            assert density_ref.close(got[b], np.array([lone, lone]), F64)
    if case == "M257":  # query 256 is the only row of chunk 1: that chunk's partial is empty
        alone = density_ref.log_density(X[256:], X[:256], hs[0])
        assert density_ref.close(got[0, 256:], alone, F64)
    if case == "dup":   # left out by index: the equal row 200 still counts for query 3, a term of ~0 (d^2 from the norms
        # is 0 up to rounding), so the density is at least that one term's -- within the bar -- and far above what the
        # other rows alone give at the narrowest bandwidth
        others = np.delete(X, [3, 200], axis=0)
        for b, h in enumerate(hs):
            floor = -np.log(M - 1) - 0.5 * D * np.log(2 * np.pi) - D * np.log(h)
            for i in (3, 200):
                assert got[b, i] >= floor - F64 * max(1.0, abs(floor)), (b, i)
            assert density_ref.close(got[b, 3:4], got[b, 200:201], F64)
        assert got[1, 3] > density_ref.log_density(X[3:4], others, hs[1])[0] + 1.0


def test_errors_and_empty():
    from phamers_amd import _lib, learning
    X, Q = _rows(20, 16, 9), _rows(5, 16, 10)
    bad_q = Q.copy()
    bad_q[2, 3] = np.nan
    with pytest.raises(ValueError):
        learning.density_sweep(bad_q, X, [0.01])
    ctx = _lib.get_context()
    out = np.empty((1, 5))
    h = np.array([0.01])
    rc = ctx.lib.phk_kde_sweep(ctx.handle, _lib.ptr(bad_q), 5, _lib.ptr(X), 20, 16, _lib.ptr(h), 1, 0, 0, _lib.ptr(out))
    assert rc == _lib.PHK_ERR_NAN
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            learning.density_sweep(Q, X, [0.01, bad])
        hb = np.array([0.01, bad])
        out2 = np.empty((2, 5))
        assert ctx.lib.phk_kde_sweep(ctx.handle, _lib.ptr(Q), 5, _lib.ptr(X), 20, 16, _lib.ptr(hb), 2, 0, 0,
                                     _lib.ptr(out2)) == _lib.PHK_ERR_ARG
    with pytest.raises(ValueError):
        learning.density_sweep(Q, X, [])
    assert ctx.lib.phk_kde_sweep(ctx.handle, _lib.ptr(Q), 5, _lib.ptr(X), 20, 16, _lib.ptr(h), 0, 0, 0,
                                 _lib.ptr(out)) == _lib.PHK_ERR_ARG
    with pytest.raises(ValueError):
        learning.density_sweep(X[:1], X[:1], [0.01], exclude_self=True)
    assert ctx.lib.phk_kde_sweep(ctx.handle, _lib.ptr(X), 1, _lib.ptr(X), 1, 16, _lib.ptr(h), 1, 1, 0,
                                 _lib.ptr(out)) == _lib.PHK_ERR_ARG
    with pytest.raises(ValueError):
        learning.density_sweep(Q, X, [0.01], exclude_self=True)
    assert ctx.lib.phk_kde_sweep(ctx.handle, _lib.ptr(Q), 5, _lib.ptr(X), 20, 16, _lib.ptr(h), 1, 1, 0,
                                 _lib.ptr(out)) == _lib.PHK_ERR_ARG
    empty = learning.density_sweep(np.empty((0, 16)), X, [0.01, 0.02, 0.03])
    assert empty.shape == (3, 0)
    with pytest.raises(ValueError):
        learning.density_sweep(Q, X, [0.01], _per_pass=_per_pass() + 1)


# ---- the real matrix ---------------------------------------------------------------------------------------------------
GRID = (0.003, 0.005, 0.01)


@pytest.fixture(scope="module")
def real():
    from oracle import oracle
    from phamers_amd import bandwidth
    ref = helpers.load_npz("ref_features.npz")
    pos = oracle.normalize_counts(ref["pos_counts"].astype(np.int64))
    neg = oracle.normalize_counts(ref["neg_counts"].astype(np.int64))
    got = bandwidth.held_out_log_densities(pos, neg, GRID, GRID, folds=None)
    table = bandwidth.grid(pos, neg, GRID, GRID)
    want = {"pos_under_pos": density_sweep_ref.log_density_sweep(pos, pos, GRID, True),
            "neg_under_pos": density_sweep_ref.log_density_sweep(neg, pos, GRID),
            "pos_under_neg": density_sweep_ref.log_density_sweep(pos, neg, GRID),
            "neg_under_neg": density_sweep_ref.log_density_sweep(neg, neg, GRID, True)}
    return pos, neg, got, table, want


def test_real_matrix_held_out_densities(real):
    pos, neg, got, table, want = real
    assert pos.shape == (2255, 256) and neg.shape == (2418, 256)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name].shape == want[name].shape, name
        assert density_ref.close(got[name], want[name], F64), name


def test_real_matrix_grid(real):
    from phamers_amd import learning
    pos, neg, got, table, want = real
    assert np.array_equal(table["positive_bandwidth"], np.repeat(GRID, 3))
    assert np.array_equal(table["negative_bandwidth"], np.tile(GRID, 3))
    for a in range(3):
        for b in range(3):
            cell = 3 * a + b
            ps, ns = got["pos_under_pos"][a] - got["pos_under_neg"][b], got["neg_under_pos"][a] - got["neg_under_neg"][b]
            assert table["auc"][cell] == learning.predictor_performance(ps, ns)[2]
            rank = density_sweep_ref.rank_auc(want["pos_under_pos"][a] - want["pos_under_neg"][b],
                                              want["neg_under_pos"][a] - want["neg_under_neg"][b])
            print("cell (%g, %g): auc %.7f, restatement %.7f" % (GRID[a], GRID[b], table["auc"][cell], rank))
            assert abs(table["auc"][cell] - rank) <= 1e-6
    best = table["best"]
    assert (table["positive_bandwidth"][best], table["negative_bandwidth"][best]) == (0.003, 0.003)
    assert table["auc"][best] == table["auc"].max()
    assert abs(table["auc"][3 * 1 + 2] - 0.9242) <= 1e-4     # the reference's defaults (0.005, 0.01)
    assert np.array_equal(table["loglik_positive"], got["pos_under_pos"].mean(axis=1))
    assert np.array_equal(table["loglik_negative"], got["neg_under_neg"].mean(axis=1))


def test_folds_agree_with_the_validator(real):
    from phamers_amd import bandwidth, cross_validate
    pos, neg = real[0][:300], real[1][:300]
    L = bandwidth.held_out_log_densities(pos, neg, [0.005], [0.01], folds=4, seed=3)
    v = cross_validate.cross_validator()
    v.positive_data, v.negative_data = pos, neg
    v.method, v.N, v.seed = 'density', 4, 3
    ps, ns = v.cross_validate()
    assert density_ref.close(L["pos_under_pos"][0] - L["pos_under_neg"][0], ps, F64)
    assert density_ref.close(L["neg_under_pos"][0] - L["neg_under_neg"][0], ns, F64)


def test_command_line(tmp_path):
    from phamers_amd import bandwidth
    ref = helpers.load_npz("ref_features.npz")
    files = []
    for tag in ("pos", "neg"):
        counts = ref[tag + "_counts"][:150].astype(np.int64)
        path = tmp_path / (tag + "_features.csv")
        with open(path, "w") as f:
            for i, row in enumerate(counts):
                f.write("%s_%d,%s\n" % (tag, i, ",".join("%d" % c for c in row)))
        files.append(str(path))
    out = str(tmp_path / "grid.csv")
    hp, hn = ["0.004", "0.01"], ["0.003", "0.01", "0.02"]
    assert bandwidth.main(["-pf", files[0], "-nf", files[1], "--positive_bandwidths"] + hp
                          + ["--negative_bandwidths"] + hn + ["-out", out]) == 0
    from phamers_amd import fileIO
    pos = fileIO.read_feature_file(files[0], normalize=True)[1]
    neg = fileIO.read_feature_file(files[1], normalize=True)[1]
    table = bandwidth.grid(pos, neg, [float(h) for h in hp], [float(h) for h in hn])
    back = bandwidth.read_grid(out)
    assert open(out).readline().startswith("# ")
    for name in bandwidth.COLUMNS:
        assert np.array_equal(back[name], table[name]), name
    assert back["best"] == table["best"]
