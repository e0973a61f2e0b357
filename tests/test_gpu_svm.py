"""GPU: the svm scoring method and phamers_amd.svm.NuSVC (svm.hip) against the reference's scikit-learn fits
(tests/golden/scoring_svm.npz, tools/gen_golden_svm.py) and the NumPy restatement (tests/svm_ref.py); the dbscan method
against the reference's scores.  Bars: the same iterations and support vectors as scikit-learn, coefficients, intercept and
decisions within 1e-6, predictions exact; bit equality across batch splits and entry points."""

import numpy as np
import pytest

from tests import helpers, svm_ref
from tests.test_svm_host import SVM_CASES, _ref_matrices, dec_tol, svm_case

pytestmark = pytest.mark.gpu
SKL = 1e-6


@pytest.fixture(scope="module")
def golden():
    return helpers.load_npz("scoring_svm.npz")


@pytest.mark.parametrize("tag", SVM_CASES)
def test_nusvc_matches_scikit_learn(golden, tag):
    from phamers_amd import svm
    g = golden
    X, y, q, gamma = svm_case(g, tag)
    m = svm.NuSVC(gamma=gamma).fit(X, y)
    assert m._gamma == float(g["gamma_" + tag])
    assert int(m.n_iter_[0]) == int(g["n_iter_" + tag][0])
    assert np.array_equal(m.support_, g["support_" + tag])
    assert np.max(np.abs(m.dual_coef_[0] - g["dual_coef_" + tag])) <= SKL
    assert abs(m.intercept_[0] - g["intercept_" + tag][0]) <= SKL
    assert np.max(np.abs(m.decision_function(q) - g["dec_" + tag])) <= dec_tol(g, tag, SKL)
    pred = m.predict(q)
    assert pred.dtype == np.float64 and np.array_equal(pred, g["pred_" + tag])
    if tag == "full":
        assert int(m.n_iter_[0]) == 1278 and len(m.support_) == 2358


@pytest.mark.parametrize("tag", SVM_CASES)
def test_decision_kernel_with_the_fixtures_coefficients(golden, tag):
    """phk_nusvc_decision fed scikit-learn's own support vectors and coefficients: within 1e-9 of the direct-difference
    restatement."""
    from phamers_amd import _lib
    g = golden
    X, _, q, _ = svm_case(g, tag)
    sv, coef, rho, gam = X[g["support_" + tag]], -g["dual_coef_" + tag], float(g["intercept_" + tag][0]), float(g["gamma_" + tag])
    got = _lib.nusvc_decision(_lib.get_context(), sv, coef, rho, gam, q)
    want = svm_ref.decision(q, sv, coef, rho, gam)
    assert np.max(np.abs(got - want)) <= dec_tol(g, tag, 1e-9)


@pytest.mark.parametrize("tag", ["full", "eq"])
def test_score_points_svm_matches_reference(golden, tag):
    """phamer_scorer.score_points and score_with_scorer (the reference's functional score_points body) give the reference's
    predictions; the functional score_points keeps its method set and still refuses svm."""
    from phamers_amd import phamer
    g = golden
    X, y, q, _ = svm_case(g, tag)
    pos, neg = X[y == 1], X[y == 0]
    got = phamer.score_with_scorer(q, pos, neg, method="svm")
    assert np.array_equal(got, g["pred_" + tag])
    with pytest.raises(NotImplementedError):
        phamer.score_points(q, pos, neg, method="svm")
    sc = phamer.phamer_scorer()
    sc.scoring_method = "svm"
    sc.data_points, sc.positive_data, sc.negative_data = q, pos, neg
    assert np.array_equal(sc.score_points(), got)


def test_svm_model_rules():
    """Scoring before a fit and infeasible fits are refused (the model keeps its last fit); svm is not OR-ed with others."""
    from phamers_amd import _lib
    pos, neg = _ref_matrices()
    q = helpers.load_npz("scoring_k4.npz")["q"][:20].copy()
    ctx = _lib.get_context()
    model = _lib.Model(ctx, pos[:300], neg[:200], k_neighbors=3)
    out = np.empty(3)
    assert ctx.lib.phk_score(ctx.handle, model.handle, _lib.ptr(q[:3]), 3, _lib.METHOD_SVM, _lib.ptr(out)) == _lib.PHK_ERR_ARG
    model.fit_svm()
    want = svm_ref.Fit(np.vstack((pos[:300], neg[:200])), np.r_[np.ones(300), np.zeros(200)]).predict(q)
    assert np.array_equal(model.score(q, "svm"), want)
    with pytest.raises(ValueError, match="infeasible"):
        model.fit_svm(nu=0.9)
    mask = np.zeros(500, np.uint8)
    mask[300:] = 1
    model.set_column_mask(mask)
    with pytest.raises(ValueError, match="greater than one"):
        model.fit_svm()
    assert np.array_equal(model.score(q, "svm"), want)
    q[4] = np.nan
    with pytest.raises(_lib.PhkError):
        model.score(q, "svm")
    model.close()


def test_masked_fit_equals_a_model_of_the_unmasked_rows():
    from phamers_amd import _lib
    pos, neg = _ref_matrices()
    q = helpers.load_npz("scoring_k4.npz")["q"]
    ctx = _lib.get_context()
    rng = np.random.default_rng(5)
    mask = (rng.random(len(pos) + len(neg)) < 0.2).astype(np.uint8)
    mp, mn = mask[:len(pos)].astype(bool), mask[len(pos):].astype(bool)
    full = _lib.Model(ctx, pos, neg, k_neighbors=3)
    full.set_column_mask(mask)
    g1 = full.fit_svm()
    alone = _lib.Model(ctx, pos[~mp], neg[~mn], k_neighbors=3)
    g2 = alone.fit_svm()
    assert g1 == g2
    Q = np.vstack((q, pos[mp][:200], neg[mn][:200]))
    assert np.array_equal(full.score(Q, "svm"), alone.score(Q, "svm"))
    full.close()
    alone.close()


def test_cross_validation_svm_resident_equals_scoring_function_path():
    from phamers_amd import cross_validate, phamer
    pos, neg = _ref_matrices()
    runs = []
    for resident in (True, False):
        v = cross_validate.cross_validator()
        v.positive_data, v.negative_data = pos, neg
        v.equalize_reference = True
        v.N = 5
        v.method = "svm"
        v.seed = 3
        if not resident:
            v.scoring_function = lambda *a, **k: phamer.score_with_scorer(*a, **k)   # (a function of its own: per-fold calls)
        runs.append(v.cross_validate())
        assert (getattr(v, "model_uploads", None) == 1) == resident
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert set(np.unique(np.concatenate(runs[0]))) <= {0.0, 1.0}


@pytest.mark.parametrize("tag", ["default", "eps0", "eps1"])
def test_dbscan_method_matches_reference(golden, tag):
    from phamers_amd import phamer
    g = golden
    pos, neg = _ref_matrices()
    q = helpers.load_npz("scoring_k4.npz")["q"]
    sc = phamer.phamer_scorer()
    sc.scoring_method = "dbscan"
    sc.eps = [float(e) for e in g["dbscan_eps_" + tag]]
    sc.data_points, sc.positive_data, sc.negative_data = q, pos, neg
    got = sc.score_points()
    want = g["dbscan_" + tag]
    assert got.shape == want.shape == (len(q), 1)
    assert np.all(np.abs(got - want) <= 1e-6 * np.maximum(1.0, np.abs(want)))


def test_dbscan_cross_validation_runs_through_the_scoring_function():
    from phamers_amd import cross_validate, phamer
    pos, neg = _ref_matrices()
    v = cross_validate.cross_validator()
    v.positive_data, v.negative_data = pos[:400], neg[:400]
    v.N = 2
    v.method = "dbscan"
    v.seed = 1
    ps, ns = v.cross_validate()
    assert ps.shape == (400,) and ns.shape == (400,) and np.all(np.abs(np.concatenate((ps, ns))) <= 1.0)
    assert v.scoring_function is phamer.score_points


def test_entry_points_and_splits_on_two_pow_20_contigs():
    """2^20 resident 5 kb contigs, count -> svm against the full reference's fit: bit-identical across the host-rows,
    resident-counts and count -> score entry points and the batch splits 1/2/4/8; 4096 sampled rows against the
    restatement's predict."""
    from oracle import oracle
    from phamers_amd import _lib, device
    pos, neg = _ref_matrices()
    ctx = _lib.get_context()
    model = _lib.Model(ctx, pos, neg, k_neighbors=3)
    model.fit_svm()
    n, L = 1 << 20, 5000
    T = n * L
    d_packed = device.DeviceArray(ctx, device.packed_words(T), np.uint32)
    d_off = device.DeviceArray(ctx, n + 1, np.uint64)
    device.synth_packed(ctx, 0, 0, n, L, d_packed, d_off)
    d_counts = device.DeviceArray(ctx, (n, 256), np.uint32)
    d_scores = device.DeviceArray(ctx, n, np.float64)
    d_status = device.DeviceArray.from_host(ctx, np.zeros(1, np.uint32))
    device.count_score(ctx, model, d_packed, None, T, d_off, n, 4, "svm", d_counts, d_scores, d_status)
    ctx.sync()
    assert d_status.to_host()[0] == 0
    full = d_scores.to_host()
    assert set(np.unique(full)) <= {0.0, 1.0}
    d_part = device.DeviceArray(ctx, n, np.float64)
    for parts in (1, 2, 4, 8):
        cuts = np.linspace(0, n, parts + 1).astype(np.int64)
        for a, b in zip(cuts[:-1], cuts[1:]):
            device.score_counts(ctx, model, d_counts.ptr + int(a) * 256 * 4, int(b - a), "svm", d_part.ptr + int(a) * 8)
        assert np.array_equal(d_part.to_host(), full), parts
    rng = np.random.default_rng(0)
    sample = np.sort(rng.choice(n, 4096, replace=False))
    counts = device.read_rows(ctx, d_counts, sample, 256)
    rows = oracle.normalize_counts(counts.astype(np.int64))
    assert np.array_equal(model.score(rows, "svm"), full[sample])           # host rows
    batch = _lib.Batch.from_counts(ctx, counts)
    assert np.array_equal(batch.score(model, "svm"), full[sample])          # resident counts
    batch.close()
    ref = svm_ref.Fit(np.vstack((pos, neg)), np.r_[np.ones(len(pos)), np.zeros(len(neg))])
    dec = ref.libsvm_decision(rows)
    clear = np.abs(dec) > 1e-9
    assert clear.mean() > 0.999
    assert np.array_equal(full[sample][clear], np.where(dec[clear] <= 0, 1.0, 0.0)[:])
    model.close()


# ---- synthetic dyadic cases: long fits, max_iter, TAU, odd shapes --------------------------------------------------------
# Every entry is a multiple of 2^-12 (or 1/8), so Q is the same on the device as in NumPy and the fit is held to scikit-learn's
# NuSVC(shrinking=False) and to the restatement within 1e-12 (tests/golden/scoring_svm_synth.npz).
from tests.test_svm_host import EXACT, synth_case, synth_ref_fit  # noqa: E402


@pytest.fixture(scope="module")
def synth():
    return helpers.load_npz("scoring_svm_synth.npz")


def _solve_launches(ctx, fn):
    """fn() with the profiler on: (its result, launches of phk_svm_solve_kernel)."""
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        out = fn()
        return out, ctx.profile().get("phk_svm_solve_kernel", (0.0, 0))[1]
    finally:
        ctx.profile_enable(False)


@pytest.mark.parametrize("case", ["long", "maxiter"])
def test_nusvc_long_fit_matches_the_unshrunk_scikit_learn_fit(synth, case):
    """~10 000 iterations (three solver launches, alpha / G / iteration carried between them; near-duplicate rows take the TAU
    branches) and max_iter = 4 097: the same iterations and support vectors as NuSVC(shrinking=False) and the restatement,
    coefficients and intercept within 1e-12, decisions within 1e-9, predictions exact."""
    from phamers_amd import _lib, svm
    s, t = synth, case + "_noshrink"
    X, y, q, nu, max_iter = synth_case(s, case)
    m, launches = _solve_launches(_lib.get_context(), lambda: svm.NuSVC(nu=nu, max_iter=max_iter).fit(X, y))
    ref = synth_ref_fit(s, case)[0]
    if case == "long":
        assert launches >= 3 and int(m.n_iter_[0]) > 2 * 4096
    assert m._gamma == float(s["gamma_" + t])
    for want_iter, want_sv, want_coef, want_b in ((int(s["n_iter_" + t][0]), s["support_" + t], s["dual_coef_" + t],
                                                   s["intercept_" + t][0]),
                                                  (int(ref.n_iter_[0]), ref.support_, ref.dual_coef_[0], ref.intercept_[0])):
        assert int(m.n_iter_[0]) == want_iter
        assert np.array_equal(m.support_, want_sv)
        assert np.max(np.abs(m.dual_coef_[0] - want_coef)) <= EXACT
        assert abs(m.intercept_[0] - want_b) <= EXACT
    assert np.max(np.abs(m.decision_function(q) - s["dec_" + t])) <= dec_tol(s, t, 1e-9)
    assert np.array_equal(m.predict(q), s["pred_" + t].astype(np.float64))


def test_nusvc_agrees_with_the_default_fit_where_scikit_learns_fits_agree(synth):
    """On a case where shrinking changes scikit-learn's solution, the device (which does not shrink) is exact against
    NuSVC(shrinking=False), and predicts as NuSVC() does wherever NuSVC() and NuSVC(shrinking=False) agree."""
    from phamers_amd import svm
    s = synth
    X, y, q, nu, _ = synth_case(s, "shrink")
    m = svm.NuSVC(nu=nu).fit(X, y)
    t = "shrink_noshrink"
    assert int(m.n_iter_[0]) == int(s["n_iter_" + t][0])
    assert np.array_equal(m.support_, s["support_" + t])
    assert np.max(np.abs(m.dual_coef_[0] - s["dual_coef_" + t])) <= EXACT
    assert abs(m.intercept_[0] - s["intercept_" + t][0]) <= EXACT
    pred = m.predict(q)
    assert np.array_equal(pred, s["pred_" + t].astype(np.float64))
    same = s["pred_shrink_default"] == s["pred_shrink_noshrink"]
    assert not same.all()
    assert np.array_equal(pred[same], s["pred_shrink_default"][same].astype(np.float64))


@pytest.mark.parametrize("max_iter", [1, 4095, 4096, 4097, 8193])
def test_max_iter_at_the_solver_launch_boundaries(synth, max_iter):
    """max_iter around the 4 096 iterations of one solver launch: 4 096 ends the first launch exactly at the limit, and the
    second must stop without a step.  Against the restatement with the same max_iter: n_iter_ = max_iter, the same support
    set, coefficients and rho within 1e-12."""
    from phamers_amd import _lib
    X, y, _, nu, _ = synth_case(synth, "long")
    ctx = _lib.get_context()
    (sv, coef, rho, it), launches = _solve_launches(
        ctx, lambda: _lib.nusvc_fit(ctx, X, y, nu, _lib.svm_gamma(X, "scale"), 1e-3, max_iter))
    ref = svm_ref.Fit(X, y, nu=nu, max_iter=max_iter)
    assert it == max_iter == int(ref.n_iter_[0])
    assert launches == max_iter // 4096 + 1
    assert np.array_equal(sv, ref.support_)
    assert np.max(np.abs(coef - ref.libsvm_coef)) <= EXACT
    assert abs(rho - ref.libsvm_rho) <= EXACT


# (n, D, positive rows or None for random labels, nu): every n around the 128-row Gram block and the 256-row chunk, D around
# the 32-column K step (D % 32 != 0: the tile kernel's FULL = false branch), imbalanced classes just inside the nu
# feasibility bound (at the bound itself the fit is refused: test_degenerate_fits_are_refused)
SVM_SHAPES = [(2, 32, None, 0.5), (3, 31, None, 0.5), (127, 33, None, 0.5), (128, 32, None, 0.5), (129, 1, None, 0.5),
              (255, 31, None, 0.5), (256, 33, 64, 0.49), (257, 32, None, 0.5), (1023, 1, None, 0.3),
              (1024, 31, 256, 0.45), (1025, 33, None, 0.5), (2049, 33, None, 0.5)]


def _shape_case(n, D, n_pos, nu):
    rng = np.random.default_rng(n * 64 + D)
    X = rng.integers(0, 8, (n, D)) / 8.0
    if n_pos is None:
        y = (X[:, 0] + rng.random(n) > 0.9).astype(np.float64)
        y[:2] = (0.0, 1.0)
    else:
        y = np.zeros(n)
        y[rng.permutation(n)[:n_pos]] = 1.0
        assert nu * n / 2 <= min(n_pos, n - n_pos)
    return X, y, rng.integers(0, 8, (300, D)) / 8.0


def test_fit_and_decision_across_shapes():
    """Fit and decision at every shape of SVM_SHAPES against the restatement: the same iterations and support set,
    coefficients and rho within 1e-12, decisions within 1e-9 (plus the cancellation term) and bit-identical whatever the
    split of the queries across calls.  The support-vector counts fall on both sides of 256 and 512 (the decision's
    256-row chunk cut)."""
    from phamers_amd import _lib
    ctx = _lib.get_context()
    counts = []
    for n, D, n_pos, nu in SVM_SHAPES:
        X, y, q = _shape_case(n, D, n_pos, nu)
        tag = (n, D, n_pos, nu)
        ref = svm_ref.Fit(X, y, nu=nu)
        sv, coef, rho, it = _lib.nusvc_fit(ctx, X, y, nu, ref._gamma, 1e-3, -1)
        assert it == int(ref.n_iter_[0]), tag
        assert np.array_equal(sv, ref.support_), tag
        assert np.max(np.abs(coef - ref.libsvm_coef)) <= EXACT, tag
        assert abs(rho - ref.libsvm_rho) <= EXACT, tag
        counts.append(len(sv))
        dec = _lib.nusvc_decision(ctx, X[sv], coef, rho, ref._gamma, q)
        want = svm_ref.decision(q, X[sv], coef, rho, ref._gamma)
        assert np.max(np.abs(dec - want)) <= 1e-9 + 1e-14 * np.abs(coef).sum(), tag
        for cut in (1, 127, 128, 129, 299):
            parts = [_lib.nusvc_decision(ctx, X[sv], coef, rho, ref._gamma, p) for p in (q[:cut], q[cut:])]
            assert np.array_equal(np.concatenate(parts), dec), (tag, cut)
    counts = np.array(counts)
    assert (counts < 256).any() and ((counts > 256) & (counts < 512)).any() and (counts > 512).any(), counts


@pytest.mark.parametrize("case", ["pair", "pair+1", "bound256", "bound1024"])
def test_degenerate_fits_are_refused(case):
    """Fits where libsvm's r is 0 or infinite, so that its coefficients or rho are not finite, and scikit-learn's fit raises:
    one row twice with labels 0 and 1 (n = 2, and n = 3 with one more row), and imbalanced classes at the exact nu
    feasibility bound nu n / 2 = min(n0, n1) (the minority at the upper bound: no free row).  The device fit raises the same
    error (it returned non-finite or no coefficients before); the restatement agrees.  A model keeps its previous svm fit."""
    from phamers_amd import _lib, svm
    X = np.array([[0.25, 0.5, 0.125], [0.25, 0.5, 0.125]])
    y = np.array([0.0, 1.0])
    nu = 0.5
    if case == "pair+1":
        X, y = np.vstack((X, [[0.5, 0.5, 0.5]])), np.array([0.0, 1.0, 1.0])
    elif case.startswith("bound"):
        n = int(case[5:])
        X, y, _ = _shape_case(n, 33 if n == 256 else 31, n // 4, 0.5)
        assert nu * n / 2 == min(y.sum(), n - y.sum())
    msg = "dual coefficients or intercepts are not finite"
    with pytest.raises(ValueError, match=msg):
        svm_ref.Fit(X, y, nu=nu)
    with pytest.raises(ValueError, match=msg):
        svm.NuSVC(nu=nu).fit(X, y)
    if case != "pair":
        return
    ctx = _lib.get_context()
    pos, neg = _ref_matrices()
    P, N = pos[:40], np.vstack((pos[:1], neg[:40]))       # negative row 0 = positive row 0
    model = _lib.Model(ctx, P, N, k_neighbors=3)
    model.fit_svm()
    q = helpers.load_npz("scoring_k4.npz")["q"][:50]
    before = model.score(q, "svm")
    mask = np.ones(len(P) + len(N), np.uint8)
    mask[[0, len(P), len(P) + 1]] = 0                     # a row twice with opposite labels, one more negative row
    model.set_column_mask(mask)
    with pytest.raises(ValueError, match=msg):
        model.fit_svm()
    assert np.array_equal(model.score(q, "svm"), before)
    model.close()
