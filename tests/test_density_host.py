"""CPU: the density method's fixture and binding, without a device."""
import numpy as np
import pytest

from tests import density_ref, helpers

SKL = 1e-9


def _ref_matrices():
    from oracle import oracle
    ref = helpers.load_npz("ref_features.npz")
    return (oracle.normalize_counts(ref["pos_counts"].astype(np.int64)),
            oracle.normalize_counts(ref["neg_counts"].astype(np.int64)))


def test_fixture_agrees_with_a_dense_float64_restatement():
    """scikit-learn's tree result (the fixture) and the dense float64 sums agree within the scikit-learn bar."""
    g = helpers.load_npz("scoring_density.npz")
    assert str(g["sklearn_version"])
    pos, neg = _ref_matrices()
    q = np.vstack((helpers.load_npz("scoring_k4.npz")["q"], g["adv_q"]))
    assert density_ref.close(g["density_full"], density_ref.density_scores(q, pos, neg), SKL)
    m = int(g["n_equalized"][0])
    assert density_ref.close(g["density_eq"], density_ref.density_scores(q, pos[:m], neg[:m]), SKL)
    for i, (hp, hn) in enumerate(g["bandwidth_pairs"]):
        assert density_ref.close(g["density_full_bw%d" % i], density_ref.density_scores(q[:100], pos, neg, hp, hn), SKL)
    pts = np.vstack((q[:10], g["adv_q"]))
    assert density_ref.close(g["get_density_pos"], density_ref.log_density(pts, pos, 0.1), SKL)
    assert density_ref.close(g["get_density_neg"], density_ref.log_density(pts, neg, 0.1), SKL)
    h = helpers.load_npz("scoring_highdim.npz")
    for k in (5, 6):
        t = "k%d" % k
        assert density_ref.close(g["density_" + t], density_ref.density_scores(h["q_" + t], h["pos_" + t], h["neg_" + t]), SKL)
    assert np.all(np.isfinite(g["density_full"]))     # the homopolymer row included (exponents ~ -2e4)


def _trees_agree(g):
    """Rows of the stored cross-validation on which the reference's KernelDensity (a KD tree on this data) and a ball tree
    agree to 1e-10 (relative).  On the others scikit-learn's tree sums are off -- one or both, by up to ~10 nats
    (tools/gen_golden_density.py); there the dense float64 sum is the yardstick."""
    return [np.abs(g["cv_%s_scores" % c] - g["cv_%s_scores_balltree" % c])
            <= 1e-10 * np.maximum(1.0, np.abs(g["cv_%s_scores_balltree" % c])) for c in ("pos", "neg")]


def test_fixture_cross_validation_is_leakage_free():
    """Each fold of the reference's seeded run equals the restatement on that fold's training rows alone, wherever
    scikit-learn's two trees agree (all but a few rows)."""
    g = helpers.load_npz("scoring_density.npz")
    pos, neg = _ref_matrices()
    seed, N, n_p, n_n = (int(x) for x in g["cv_meta"])
    P, Nm = pos[:n_p], neg[:n_n]
    pa, na = g["cv_pos_asmt"], g["cv_neg_asmt"]
    from phamers_amd import cross_validate
    plan = cross_validate.FoldPlan(n_p, n_n, N, seed)
    assert np.array_equal(plan.positive, pa) and np.array_equal(plan.negative, na)
    ok_p, ok_n = _trees_agree(g)
    assert ok_p.sum() + ok_n.sum() >= 0.97 * (n_p + n_n)
    for fold in range(N):
        op, on = pa == fold, na == fold
        want = density_ref.density_scores(np.vstack((P[op], Nm[on])), P[~op], Nm[~on])
        ref = np.concatenate((g["cv_pos_scores"][op], g["cv_neg_scores"][on]))
        ok = np.concatenate((ok_p[op], ok_n[on]))
        assert density_ref.close(ref[ok], want[ok], SKL)


def test_binding_declares_the_density_entries():
    from phamers_amd import _lib
    assert _lib.METHODS["density"] == _lib.METHOD_DENSITY == 4
    c_int, c_double = _lib.c_int, _lib.c_double
    res, args = _lib.SIGNATURES["phk_model_set_bandwidths"]
    assert res is c_int and args[2:] == [c_double, c_double]
    res, args = _lib.SIGNATURES["phk_kde_log_density"]
    assert res is c_int and len(args) == 8 and args[6] is c_double
    text = open(helpers.os.path.join(helpers.REPO, "include", "phamers_hip.h")).read()
    assert "#define PHK_METHOD_DENSITY 4" in text


@pytest.mark.parametrize("method", ["svm", "dbscan", "silhouette"])
def test_other_methods_still_raise_before_device_work(method, monkeypatch):
    from phamers_amd import _lib, phamer

    def no_device(*a, **k):
        raise AssertionError("device work for an unimplemented method")
    monkeypatch.setattr(_lib, "get_context", no_device)
    monkeypatch.setattr(_lib, "Model", no_device)
    q = helpers.load_npz("scoring_k4.npz")["q"][:4]
    with pytest.raises(NotImplementedError):
        phamer.score_points(q, q, q, method=method)


def test_density_is_a_scoring_method_of_the_facade():
    from phamers_amd import phamer
    sc = phamer.phamer_scorer()
    assert sc.method_function_map["density"] == sc.density_score_points
    assert (sc.positive_bandwidth, sc.negative_bandwidth) == (0.005, 0.01)
