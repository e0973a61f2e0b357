"""CPU-only: the restatement the GPU tests of the density bandwidth sweep rest on (tests/density_sweep_ref.py) against its own
definition and against scikit-learn (tests/golden/density_sweep.npz, tools/gen_golden_density_sweep.py), the bandwidth
grid's cell order, tie rule and CSV round trip on top of the restatement, and the argument errors that are raised before
any device work."""
import numpy as np
import pytest

from tests import density_ref, density_sweep_ref, helpers

SKL = 1e-9


def _rows(n, D, seed):
    rng = np.random.default_rng(seed)
    base = rng.random(D) + 0.5
    x = base[None, :] * (1.0 + 0.3 * rng.standard_normal((n, D))).clip(0.05)
    return x / x.sum(axis=1, keepdims=True)


def test_leave_one_out_restatement_is_the_fit_without_the_row():
    # 1e-12 absolute: the two sides form q.X with different matrix shapes, so their d^2 differ by rounding, at most
    # (D + 2) u (|q|^2 + |r|^2 + 2 |q.r|) = 18 * 1.1e-16 * 4 * 0.07 = 5.5e-16 on these rows, times 1 / 2 h^2 in the exponent:
    # 6.9e-13 at h = 0.02 (1.7e-11 at h = 0.004, which is why no narrower bandwidth is asked to meet this bar)
    X = _rows(40, 16, 0)
    hs = [0.02, 0.05, 0.3]
    got = density_sweep_ref.log_density_sweep(X, X, hs, exclude_self=True)
    assert got.shape == (3, 40)
    for b, h in enumerate(hs):
        for i in range(40):
            want = density_ref.log_density(X[i:i + 1], np.delete(X, i, 0), h)[0]
            assert abs(got[b, i] - want) <= 1e-12, (b, i)
    plain = density_sweep_ref.log_density_sweep(X[:5], X, hs)
    assert np.array_equal(plain[1], density_ref.log_density(X[:5], X, hs[1]))


def test_restatement_matches_scikit_learn():
    g = helpers.load_npz("density_sweep.npz")
    X, Q, hs = g["X"], g["Q"], g["bandwidths"]
    assert X.shape == (200, 32) and Q.shape == (64, 32) and len(hs) == 3
    got = density_sweep_ref.log_density_sweep(Q, X, hs)
    agree = np.abs(g["sweep_kd_tree"] - g["sweep_ball_tree"]) <= 1e-10
    assert agree.sum(axis=1).min() >= 16     # the comparison is not vacuous at any bandwidth
    assert density_ref.close(got[agree], g["sweep_kd_tree"][agree], SKL)
    loo = density_sweep_ref.log_density_sweep(X[:40], X[:40], hs, exclude_self=True)
    agree = np.abs(g["loo_kd_tree"] - g["loo_ball_tree"]) <= 1e-10
    assert agree.sum(axis=1).min() >= 10
    assert density_ref.close(loo[agree], g["loo_kd_tree"][agree], SKL)


def test_rank_auc():
    assert density_sweep_ref.rank_auc([3.0, 2.0], [1.0, 0.0]) == 1.0
    assert density_sweep_ref.rank_auc([0.0], [1.0, 2.0]) == 0.0
    assert density_sweep_ref.rank_auc([1.0, 1.0], [1.0]) == 0.5
    assert density_sweep_ref.rank_auc([2.0, 0.0], [1.0]) == 0.5
    rng = np.random.default_rng(1)
    p, n = rng.standard_normal(50) + 1, rng.standard_normal(70)
    brute = ((p[:, None] > n[None, :]).sum() + 0.5 * (p[:, None] == n[None, :]).sum()) / (50.0 * 70.0)
    assert abs(density_sweep_ref.rank_auc(p, n) - brute) < 1e-15


@pytest.fixture
def on_restatement(monkeypatch):
    """learning.density_sweep and learning.predictor_performance served by the restatement: no library is touched."""
    from phamers_amd import learning
    calls = []

    def sweep(queries, data, bandwidths, exclude_self=False, **kw):
        calls.append((np.asarray(queries).shape, np.asarray(data).shape, tuple(bandwidths), bool(exclude_self)))
        return density_sweep_ref.log_density_sweep(queries, data, list(bandwidths), exclude_self)

    def performance(positive_scores, negative_scores):
        return None, None, density_sweep_ref.rank_auc(positive_scores, negative_scores)

    monkeypatch.setattr(learning, "density_sweep", sweep)
    monkeypatch.setattr(learning, "predictor_performance", performance)
    return calls


def test_grid_cell_order_and_best(on_restatement):
    from phamers_amd import bandwidth
    pos, neg = _rows(60, 16, 2), _rows(50, 16, 3) ** 1.3
    neg /= neg.sum(axis=1, keepdims=True)
    hp, hn = [0.05, 0.01, 0.05], [0.02, 0.1]
    L = bandwidth.held_out_log_densities(pos, neg, hp, hn)
    assert on_restatement == [((60, 16), (60, 16), tuple(hp), True), ((50, 16), (60, 16), tuple(hp), False),
                              ((60, 16), (50, 16), tuple(hn), False), ((50, 16), (50, 16), tuple(hn), True)]
    assert sorted(L) == sorted(bandwidth.ARRAYS)
    assert L["pos_under_pos"].shape == (3, 60) and L["neg_under_pos"].shape == (3, 50)
    assert L["pos_under_neg"].shape == (2, 60) and L["neg_under_neg"].shape == (2, 50)
    t = bandwidth.grid(pos, neg, hp, hn)
    assert t["positive_bandwidth"].tolist() == [0.05, 0.05, 0.01, 0.01, 0.05, 0.05]
    assert t["negative_bandwidth"].tolist() == [0.02, 0.1, 0.02, 0.1, 0.02, 0.1]
    for a in range(3):
        for b in range(2):
            want = density_sweep_ref.rank_auc(L["pos_under_pos"][a] - L["pos_under_neg"][b],
                                              L["neg_under_pos"][a] - L["neg_under_neg"][b])
            assert t["auc"][2 * a + b] == want
    # the repeated h+ gives two equal rows of cells; the first cell of the largest area wins
    assert np.array_equal(t["auc"][0:2], t["auc"][4:6])
    assert t["best"] == int(np.flatnonzero(t["auc"] == t["auc"].max())[0])
    if t["auc"][:2].max() == t["auc"].max():
        assert t["best"] < 2
    assert np.array_equal(t["loglik_positive"], L["pos_under_pos"].mean(axis=1))
    assert np.array_equal(t["loglik_negative"], L["neg_under_neg"].mean(axis=1))


def test_best_breaks_ties_by_grid_order(on_restatement):
    from phamers_amd import bandwidth
    pos, neg = _rows(30, 8, 4), _rows(30, 8, 5)
    t = bandwidth.grid(pos, neg, [0.03, 0.03], [0.03, 0.03])     # four identical cells
    assert len(set(t["auc"].tolist())) == 1 and t["best"] == 0


def test_folds_use_the_validators_split(on_restatement):
    from phamers_amd import bandwidth, cross_validate
    pos, neg = _rows(23, 8, 6), _rows(17, 8, 7)
    L = bandwidth.held_out_log_densities(pos, neg, [0.02], [0.04, 0.01], folds=3, seed=5)
    assert len(on_restatement) == 12 and not any(c[3] for c in on_restatement)
    plan = cross_validate.FoldPlan(23, 17, 3, 5)
    for fold in range(3):
        out_p, out_n = plan.held_out(fold)
        assert np.array_equal(L["pos_under_pos"][0, out_p], density_ref.log_density(pos[out_p], pos[~out_p], 0.02))
        assert np.array_equal(L["neg_under_neg"][1, out_n], density_ref.log_density(neg[out_n], neg[~out_n], 0.01))
        assert np.array_equal(L["neg_under_pos"][0, out_n], density_ref.log_density(neg[out_n], pos[~out_p], 0.02))
        assert np.array_equal(L["pos_under_neg"][0, out_p], density_ref.log_density(pos[out_p], neg[~out_n], 0.04))


def test_csv_round_trip(on_restatement, tmp_path):
    from phamers_amd import bandwidth
    pos, neg = _rows(30, 8, 8), _rows(25, 8, 9)
    t = bandwidth.grid(pos, neg, [0.1 / 3, 0.007], [0.02, 1e-3, 0.3])
    path = str(tmp_path / "grid.csv")
    bandwidth.save_grid(path, t)
    lines = open(path).read().splitlines()
    assert lines[0] == "# Density bandwidth grid: positive_bandwidth,negative_bandwidth,auc"
    assert len(lines) == 7 and lines[1].split(",")[0] == repr(0.1 / 3)
    back = bandwidth.read_grid(path)
    for name in bandwidth.COLUMNS:
        assert np.array_equal(back[name], t[name]), name
    assert back["best"] == t["best"]


def test_argument_errors_need_no_library(monkeypatch):
    from phamers_amd import _lib, bandwidth, learning

    def no_library(*a, **kw):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "get_context", no_library)
    X, Q = _rows(6, 8, 10), _rows(3, 8, 11)
    bad_q = Q.copy()
    bad_q[1, 2] = np.nan
    bad_x = X.copy()
    bad_x[0, 0] = np.nan
    for args, kw in (((bad_q, X, [0.01]), {}), ((Q, bad_x, [0.01]), {}), ((Q, X, []), {}),
                     ((Q, X, [0.01, 0.0]), {}), ((Q, X, [-1.0]), {}), ((Q, X, [float("inf")]), {}),
                     ((Q, X, [float("nan")]), {}), ((Q, X, [0.01]), {"exclude_self": True}),
                     ((X[:1], X[:1], [0.01]), {"exclude_self": True}),
                     ((Q, X, [0.01]), {"_per_pass": 0}), ((Q, X, [0.01]), {"_per_pass": learning.DENSITY_SWEEP_PER_PASS + 1})):
        with pytest.raises(ValueError):
            learning.density_sweep(*args, **kw)
    for hp, hn in (([], [0.01]), ([0.01], []), ([0.0], [0.01]), ([0.01], [float("nan")])):
        with pytest.raises(ValueError):
            bandwidth.held_out_log_densities(X, Q, hp, hn)
    with pytest.raises(ValueError):
        bandwidth.grid(bad_x, Q, [0.01], [0.01])


def test_per_pass_constant_matches_the_header():
    import os
    import re
    from phamers_amd import _lib, learning
    text = open(os.path.join(helpers.REPO, "include", "phamers_hip.h")).read()
    value = int(re.search(r"#define\s+PHK_KDE_SWEEP_PER_PASS\s+(\d+)", text).group(1))
    assert learning.DENSITY_SWEEP_PER_PASS == _lib.KDE_SWEEP_PER_PASS == value


# ---- the inputs of tests/test_gpu_density_sweep_shapes.py ---------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 32])
def test_grid_rows_tie_at_the_minimum(D):
    Q, X = density_sweep_ref.grid_rows(D, 40 + D)
    assert Q.shape == (130, D) and X.shape == (300, D)
    for a in (Q, X):
        assert np.array_equal(a * 8.0, np.round(a * 8.0)) and a.min() == 0.0 and a.max() == 0.25
    assert np.array_equal(X[255], X[256]) and np.array_equal(X[16], X[17])
    assert not np.array_equal(X[254], X[255]) and not np.array_equal(X[15], X[16])
    # every d^2 is the true one: an integer multiple of 1/64 below 2^53 / 64 however it is summed
    d2 = ((Q[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    gram = np.einsum("ij,ij->i", Q, Q)[:, None] + np.einsum("ij,ij->i", X, X)[None, :] - 2.0 * (Q @ X.T)
    assert np.array_equal(d2, gram) and np.array_equal(d2 * 64.0, np.round(d2 * 64.0))
    assert (d2[:40].min(axis=1) == 0.0).all() and d2[0, 16] == d2[0, 17] == 0.0 and d2[1, 255] == d2[1, 256] == 0.0
    at_min = density_sweep_ref.rows_at_the_minimum(Q, X)
    assert np.array_equal(at_min, (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1))
    print("D = %d: %d of 130 queries attain their smallest d^2 twice or more (most: %d rows)" % (D, (at_min >= 2).sum(), at_min.max()))
    assert 2 * (at_min >= 2).sum() >= 130
    own = density_sweep_ref.rows_at_the_minimum(X, X, exclude_self=True)
    assert own[255] >= 1 and own[16] >= 1 and (own >= 2).any()


def test_near_tie_rows_differ_by_one_ulp_in_one_column():
    Q, X = density_sweep_ref.near_tie_rows(32, 82)
    assert np.array_equal(density_sweep_ref.smooth_rows(20, 7, 3), _rows(20, 7, 3))
    differ = X[1::2] != X[0::2]
    assert (differ.sum(axis=1) == 1).all() and len(set(np.argmax(differ, axis=1).tolist())) == 32
    assert np.array_equal(X[1::2][differ], np.nextafter(X[0::2][differ], 1.0))
    assert np.array_equal(Q[:40], X[0:80:2]) and not (Q[40:, None, :] == X[None, :, :]).all(axis=2).any()
