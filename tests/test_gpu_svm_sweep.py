"""GPU: the NuSVC nu x gamma sweep (svm_sweep.hip, svm.nusvc_sweep, phamers_amd.svm_grid) against the single fits it batches
(svm.NuSVC: every number with array_equal) and against the restatement (tests/svm_sweep_ref.py, the bars of
tests/test_gpu_svm.py: the same iterations and support, coefficients and intercept within 1e-12 on dyadic data, decisions
within 1e-9 plus the cancellation term)."""
import numpy as np
import pytest

from tests import helpers, svm_sweep_ref
from tests.test_svm_host import EXACT, _ref_matrices, synth_case

pytestmark = pytest.mark.gpu

OK, INFEASIBLE, NOT_FINITE = svm_sweep_ref.OK, svm_sweep_ref.INFEASIBLE, svm_sweep_ref.NOT_FINITE


def single_fit(X, y, nu, gamma, tol=1e-3, max_iter=-1):
    from phamers_amd import svm
    return svm.NuSVC(nu=nu, gamma=gamma, tol=tol, max_iter=max_iter).fit(X, y)


def assert_fit_equal(tag, status, n_iter, n_support, intercept, dual_coef, X, y, rows, nu, gamma, max_iter=-1):
    """A problem of the sweep (its dense coefficients over all n rows) against svm.NuSVC on the rows ``rows`` (a mask or
    None): the same status, and for a fit the same n_iter_, support_, dual_coef_ and intercept_, bit for bit.  Returns the
    single fit (None where it raises)."""
    Xs, ys = (X, y) if rows is None else (X[rows], y[rows])
    m, st = svm_sweep_ref.fit_or_status(single_fit, Xs, ys, nu, gamma, 1e-3, max_iter)
    assert status == st, (tag, status, st)
    if m is None:
        assert np.isnan(intercept) and np.isnan(dual_coef).all(), tag
        return None
    assert n_iter == int(m.n_iter_[0]), (tag, n_iter, int(m.n_iter_[0]))
    assert n_support == len(m.support_), tag
    want = svm_sweep_ref.dense_coef(m, len(y), rows)
    assert np.array_equal(np.flatnonzero(dual_coef), np.sort(np.flatnonzero(want))), tag
    assert np.array_equal(dual_coef, want), tag
    assert intercept == m.intercept_[0], tag
    return m


def assert_sweep_equals_the_loop(res, X, y, folds, max_iter=-1, cells=None, fold_subset=None):
    """Every problem of ``res`` against its single fit, the held-out decisions against decision_function, and the cell
    fields against the problems' statuses.  Returns {(g, v): [status of the full fit, of fold 0, ...]}."""
    seen = {}
    for g, gamma in enumerate(res.gammas):
        for v, nu in enumerate(res.nus):
            if cells is not None and (g, v) not in cells:
                continue
            sts = []
            # the cell fields are NaN when any problem of the cell has a status: compare the problems through the fold fields
            full_m, full_st = svm_sweep_ref.fit_or_status(single_fit, X, y, nu, gamma, 1e-3, max_iter)
            sts.append(full_st)
            fold_fits = []
            for f in range(folds or 0):
                if fold_subset is not None and f not in fold_subset:
                    continue
                held = res.fold_of == f
                m = assert_fit_equal((g, v, f), int(res.fold_status[g, v, f]), int(res.fold_n_iter[g, v, f]),
                                     int(res.fold_n_support[g, v, f]), res.fold_intercept[g, v, f], res.fold_dual_coef[g, v, f],
                                     X, y, ~held, nu, gamma, max_iter)
                sts.append(OK if m is not None else int(res.fold_status[g, v, f]))
                fold_fits.append((m, held))
            want_status = next((s for s in sts if s), 0) if fold_subset is None else int(res.status[g, v])
            assert int(res.status[g, v]) == want_status, (g, v, sts)
            if res.status[g, v] != 0:
                assert np.isnan(res.intercept[g, v]) and np.isnan(res.dual_coef[g, v]).all(), (g, v)
                if folds:
                    assert np.isnan(res.held_decision[g, v]).all() and np.isnan(res.held_predict[g, v]).all(), (g, v)
                    assert np.isnan(res.auc[g, v]) and np.isnan(res.accuracy[g, v]), (g, v)
            else:
                assert int(res.n_iter[g, v]) == int(full_m.n_iter_[0]), (g, v)
                assert int(res.n_support[g, v]) == len(full_m.support_), (g, v)
                assert np.array_equal(res.dual_coef[g, v], svm_sweep_ref.dense_coef(full_m, len(y))), (g, v)
                assert res.intercept[g, v] == full_m.intercept_[0], (g, v)
                for m, held in fold_fits:
                    assert np.array_equal(res.held_decision[g, v][held], m.decision_function(X[held])), (g, v)
                    assert np.array_equal(res.held_predict[g, v][held], m.predict(X[held])), (g, v)
            seen[(g, v)] = sts
    return seen


# ---- 1. the grid every later test reuses -----------------------------------------------------------------------------------
GAMMAS1, NUS1, FOLDS1, SEED1 = (0.5, 2.0, 8.0), (0.1, 0.3, 0.5, 0.7), 4, 2


def grid1_data():
    """180 + 120 rows x 17 with entries k / 8, a fifth of the labels flipped: 23 rows of the larger class and 38 of the smaller,
    which leaves 195 + 105 rows -- nu = 0.7 is then feasible on all rows (at the bound: 0.7 * 300 / 2 = 105) and on the folds
    that hold out 26 rows of the smaller class and 49 of the larger, and infeasible on the other folds."""
    rng = np.random.default_rng(17)
    X = np.vstack((rng.integers(0, 6, (180, 17)), rng.integers(2, 8, (120, 17)))) / 8.0
    y = np.r_[np.ones(180), np.zeros(120)]
    flip = np.r_[rng.permutation(180)[:23], 180 + rng.permutation(120)[:38]]
    y[flip] = 1 - y[flip]
    keep = rng.permutation(300)
    return X[keep], y[keep]


@pytest.fixture(scope="module")
def grid1():
    from phamers_amd import svm
    X, y = grid1_data()
    return X, y, svm.nusvc_sweep(X, y, NUS1, GAMMAS1, folds=FOLDS1, seed=SEED1)


def results_equal(a, b, folds=True):
    names = ["status", "n_iter", "n_support", "intercept", "dual_coef"]
    if folds:
        names += ["fold_status", "fold_n_iter", "fold_n_support", "fold_intercept", "fold_dual_coef", "held_decision",
                  "held_predict", "auc", "accuracy"]
    for name in names:
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name


def test_every_cell_equals_its_single_fit(grid1):
    X, y, res = grid1
    assert (int(y.sum()), len(y)) == (195, 300)
    assert res.status.shape == res.auc.shape == (3, 4) and res.held_decision.shape == (3, 4, 300)
    assert res.fold_n_iter.shape == (3, 4, 4) and res.dual_coef.shape == (3, 4, 300)
    seen = assert_sweep_equals_the_loop(res, X, y, FOLDS1)
    # nu = 0.7: some folds infeasible, others not -- exactly where the single fit raises -- and no other column has a status
    for g in range(3):
        sts = seen[(g, 3)]
        assert INFEASIBLE in sts[1:] and OK in sts[1:], sts
        assert res.status[g, 3] != 0
        assert (res.status[g, :3] == 0).all() and (res.fold_status[g, :3] == 0).all()
    alive = res.status == 0
    assert ((res.auc[alive] > 0.5) & (res.auc[alive] <= 1.0)).all() and ((res.accuracy[alive] > 0.5) & (res.accuracy[alive] <= 1)).all()
    assert set(np.unique(res.held_predict[alive])) <= {0.0, 1.0}
    assert np.array_equal(res.classes_, [0.0, 1.0])


def test_grid_against_the_restatement(grid1):
    """The bars of tests/test_gpu_svm.py on dyadic data: iterations and support equal, coefficients and intercept within
    1e-12, held-out decisions within 1e-9 plus 1e-14 of the sum of |coefficients|."""
    X, y, res = grid1
    ref = svm_sweep_ref.sweep(X, y, NUS1, GAMMAS1, FOLDS1, SEED1)
    for (g, v), cell in ref.items():
        m, st = cell["full"]
        sts = [st] + [s for _, s, _ in cell["folds"]]
        assert int(res.status[g, v]) == next((s for s in sts if s), 0), (g, v)
        for f, (fm, fst, held) in enumerate(cell["folds"]):
            assert int(res.fold_status[g, v, f]) == fst, (g, v, f)
            if fm is None:
                continue
            assert int(res.fold_n_iter[g, v, f]) == int(fm.n_iter_[0]), (g, v, f)
            want = svm_sweep_ref.dense_coef(fm, len(y), ~held)
            assert np.array_equal(np.flatnonzero(res.fold_dual_coef[g, v, f]), np.flatnonzero(want)), (g, v, f)
            assert np.max(np.abs(res.fold_dual_coef[g, v, f] - want)) <= EXACT, (g, v, f)
            assert abs(res.fold_intercept[g, v, f] - fm.intercept_[0]) <= EXACT, (g, v, f)
        if res.status[g, v] != 0:
            continue
        assert int(res.n_iter[g, v]) == int(m.n_iter_[0]), (g, v)
        assert np.max(np.abs(res.dual_coef[g, v] - svm_sweep_ref.dense_coef(m, len(y)))) <= EXACT, (g, v)
        assert abs(res.intercept[g, v] - m.intercept_[0]) <= EXACT, (g, v)
        tol = 1e-9 + 1e-14 * max(np.abs(fm.dual_coef_).sum() for fm, _, _ in cell["folds"])
        assert np.max(np.abs(res.held_decision[g, v] - cell["held_decision"])) <= tol, (g, v)


# ---- 2. shapes ---------------------------------------------------------------------------------------------------------------
SHAPES = list(zip((2, 3, 64, 65, 1023, 1024, 1025, 2049), (1, 31, 32, 33, 1, 31, 32, 33)))


def shape_case(n, D):
    rng = np.random.default_rng(n * 64 + D)
    X = rng.integers(0, 8, (n, D)) / 8.0
    y = (X[:, 0] + rng.random(n) > 0.9).astype(np.float64)
    y[:2] = (0.0, 1.0)
    return X, y


@pytest.mark.parametrize("n,D", SHAPES)
def test_shapes(n, D):
    """Rows around the 128-row Gram block, the 256-row chunk and the solver's rows per thread, columns around the 32-column
    K step; two folds where both classes keep two rows or more."""
    from phamers_amd import svm
    X, y = shape_case(n, D)
    folds = 2 if min(y.sum(), n - y.sum()) >= 4 else None
    assert (folds is None) == (n <= 3)
    res = svm.nusvc_sweep(X, y, (0.3, 0.5), (1.0 / D,), folds=folds, seed=n)
    seen = assert_sweep_equals_the_loop(res, X, y, folds)
    assert any(all(s == OK for s in sts) for sts in seen.values()) or n <= 3


# ---- 3. more problems than compute units ---------------------------------------------------------------------------------------
def test_more_problems_than_compute_units():
    from phamers_amd import svm
    rng = np.random.default_rng(96)
    X = rng.integers(0, 8, (96, 8)) / 8.0
    y = (X[:, 0] + X[:, 1] + 0.6 * rng.random(96) > 1.2).astype(np.float64)
    gammas, nus = (0.25, 1.0, 4.0, 16.0), (0.1, 0.2, 0.3, 0.4, 0.5)
    res = svm.nusvc_sweep(X, y, nus, gammas, folds=15, seed=5)
    assert res.fold_status.size + res.status.size == 320
    seen = assert_sweep_equals_the_loop(res, X, y, 15)
    assert sum(all(s == OK for s in sts) for sts in seen.values()) >= 12


# ---- 4. several launches, uneven problems ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_case():
    X, y, _, nu, _ = synth_case(helpers.load_npz("scoring_svm_synth.npz"), "long")
    from phamers_amd import _lib
    return X, y, nu, _lib.svm_gamma(X, "scale")


def sweep_launches(fn):
    from phamers_amd import _lib
    ctx = _lib.get_context()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        out = fn()
        return out, ctx.profile().get("phk_svm_sweep_solve_kernel", (0.0, 0))[1]
    finally:
        ctx.profile_enable(False)


LONG_NUS = (0.5, 0.9, 0.95)   # at gamma = 'scale': about 10 000, 400 and 200 iterations


def test_a_long_cell_among_short_ones(long_case):
    from phamers_amd import svm
    X, y, nu, scale = long_case
    assert nu == LONG_NUS[0]
    res, launches = sweep_launches(lambda: svm.nusvc_sweep(X, y, LONG_NUS, (scale,)))
    assert res.n_iter[0, 0] > 2 * 4096 and launches >= 3
    assert (res.n_iter[0, 1:] < 1000).all() and (res.n_iter[0, 1:] > 0).all(), res.n_iter
    assert_sweep_equals_the_loop(res, X, y, None)


@pytest.mark.parametrize("max_iter", [4095, 4096, 4097])
def test_max_iter_holds_per_problem(long_case, max_iter):
    from phamers_amd import svm
    X, y, nu, scale = long_case
    res, launches = sweep_launches(lambda: svm.nusvc_sweep(X, y, LONG_NUS[:2], (scale,), max_iter=max_iter))
    assert res.n_iter[0, 0] == max_iter and 0 < res.n_iter[0, 1] < 1000
    assert launches == max_iter // 4096 + 1
    assert_sweep_equals_the_loop(res, X, y, None, max_iter=max_iter)


# ---- 5. state routes -------------------------------------------------------------------------------------------------------------
def test_global_state_route_equals_the_lds_route(grid1):
    from phamers_amd import svm
    X, y, res = grid1
    results_equal(svm.nusvc_sweep(X, y, NUS1, GAMMAS1, folds=FOLDS1, seed=SEED1, _lds_rows=0), res)
    results_equal(svm.nusvc_sweep(X, y, NUS1, GAMMAS1, folds=FOLDS1, seed=SEED1, _lds_rows=299), res)   # (n = 300: global)
    for threads in (64, 256, 1024):
        results_equal(svm.nusvc_sweep(X, y, NUS1, GAMMAS1, folds=FOLDS1, seed=SEED1, _threads=threads), res)


@pytest.mark.parametrize("extra", [0, 1])
def test_at_the_lds_capacity_and_one_row_past_it(extra):
    from phamers_amd import _lib, svm
    n = _lib.nusvc_sweep_lds_rows() + extra
    assert 160 * 1024 - 1024 - 17 < 17 * _lib.nusvc_sweep_lds_rows() <= 160 * 1024 - 1024
    rng = np.random.default_rng(n)
    X = rng.integers(0, 8, (n, 8)) / 8.0
    y = (X[:, 0] + X[:, 1] + rng.random(n) > 1.3).astype(np.float64)
    res = svm.nusvc_sweep(X, y, (0.4,), (0.5,))
    assert res.status[0, 0] == OK
    assert_sweep_equals_the_loop(res, X, y, None)


# ---- 6. pass split ---------------------------------------------------------------------------------------------------------------
def test_one_gamma_per_pass_equals_the_default(grid1):
    from phamers_amd import svm
    X, y, res = grid1
    for per in (1, 2):
        results_equal(svm.nusvc_sweep(X, y, NUS1, GAMMAS1, folds=FOLDS1, seed=SEED1, _gammas_per_pass=per), res)


# ---- 7. degenerate cells ---------------------------------------------------------------------------------------------------------
def test_a_non_finite_fit_gets_a_status():
    """Two identical rows with opposite labels and nothing else: libsvm's r is 0, the single fit raises."""
    from phamers_amd import svm
    X = np.array([[0.25, 0.5, 0.125], [0.25, 0.5, 0.125]])
    y = np.array([0.0, 1.0])
    with pytest.raises(ValueError, match="not finite"):
        single_fit(X, y, 0.5, 1.0)
    res = svm.nusvc_sweep(X, y, (0.5, 1.0), (1.0, 4.0))
    assert (res.status == NOT_FINITE).all()
    assert np.isnan(res.intercept).all() and np.isnan(res.dual_coef).all()


def test_a_fold_without_a_class_is_infeasible_and_alone_in_it():
    """One row of class 1: the fold that holds it out has no row of that class and is infeasible in every cell; the other
    folds and the fits on all rows are solved as the single fits are."""
    from phamers_amd import svm
    rng = np.random.default_rng(3)
    X = rng.integers(0, 8, (41, 5)) / 8.0
    y = np.zeros(41)
    y[7] = 1.0
    res = svm.nusvc_sweep(X, y, (0.02, 0.04), (1.0, 8.0), folds=4, seed=0)
    lost = int(res.fold_of[7])
    assert (res.fold_status[:, :, lost] == INFEASIBLE).all()
    assert (np.delete(res.fold_status, lost, axis=2) != INFEASIBLE).all()
    assert (res.status != OK).all()          # (every cell has that fold)
    assert_sweep_equals_the_loop(res, X, y, 4)


# ---- 8. the reference rows -------------------------------------------------------------------------------------------------------
def test_reference_rows():
    from phamers_amd import _lib, svm
    pos, neg = _ref_matrices()
    assert (len(pos), len(neg)) == (2255, 2418)
    X = np.vstack((pos, neg))
    y = np.r_[np.ones(len(pos)), np.zeros(len(neg))]
    scale = _lib.svm_gamma(X, "scale")
    res = svm.nusvc_sweep(X, y, (0.25, 0.5), [scale / 4, "scale", scale * 4], folds=5, seed=0)
    assert res.gammas[1] == scale and (res.status == 0).all()
    assert int(res.n_iter[1, 1]) == 1278 and int(res.n_support[1, 1]) == 2358
    assert ((res.auc > 0.8) & (res.auc < 1.0)).all()
    assert_sweep_equals_the_loop(res, X, y, 5, cells={(1, 1)}, fold_subset={3})
    assert_sweep_equals_the_loop(res, X, y, 5, cells={(2, 0)}, fold_subset={0})


# ---- 9. through the validator ----------------------------------------------------------------------------------------------------
def test_the_validator_reproduces_a_cell_and_keeps_its_defaults():
    from phamers_amd import _lib, cross_validate, svm
    pos, neg = _ref_matrices()
    pos, neg = pos[:300], neg[:200]
    X = np.vstack((pos, neg))
    y = np.r_[np.ones(len(pos)), np.zeros(len(neg))]
    scale = _lib.svm_gamma(X, "scale")
    res = svm.nusvc_sweep(X, y, (0.2, 0.4), (scale / 2, scale * 2), folds=3, seed=6)
    assert (res.status == 0).all()

    def validator():
        v = cross_validate.cross_validator()
        v.positive_data, v.negative_data, v.N, v.method, v.seed = pos, neg, 3, "svm", 6
        return v
    for g, k in ((0, 1), (1, 0)):
        v = validator()
        v.svm_gamma, v.svm_nu = res.cell(g, k)
        ps, ns = v.cross_validate()
        assert set(np.unique(np.r_[ps, ns])) <= {0.0, 1.0}
        assert np.array_equal(ps, res.held_predict[g, k][:300]) and np.array_equal(ns, res.held_predict[g, k][300:])
    # the defaults: what model.fit_svm() without arguments gives, fold by fold
    v = validator()
    ps, ns = v.cross_validate()
    plan = cross_validate.FoldPlan(300, 200, 3, 6)
    model = _lib.Model(_lib.get_context(), pos, neg, k_neighbors=3)
    want_p, want_n = np.zeros(300), np.zeros(200)
    for fold in range(3):
        out_p, out_n = plan.held_out(fold)
        model.set_column_mask(np.concatenate((out_p, out_n)))
        model.fit_svm()
        s = model.score(np.vstack((pos[out_p], neg[out_n])), "svm")
        want_p[out_p], want_n[out_n] = s[:out_p.sum()], s[out_p.sum():]
    model.close()
    assert np.array_equal(ps, want_p) and np.array_equal(ns, want_n)


# ---- 10. command line ----------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path):
    from phamers_amd import _lib, fileIO, svm_grid
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
    assert svm_grid.main(["-pf", files[0], "-nf", files[1], "--nu", "0.2", "0.5", "--gamma", "300", "--gamma_scale", "0.5", "2",
                          "-N", "3", "--seed", "1", "-out", out]) == 0
    pos = fileIO.read_feature_file(files[0], normalize=True)[1]
    neg = fileIO.read_feature_file(files[1], normalize=True)[1]
    scale = _lib.svm_gamma(np.vstack((pos, neg)), "scale")
    table = svm_grid.grid(pos, neg, [0.2, 0.5], [300.0, 0.5 * scale, 2 * scale], folds=3, seed=1)
    back = svm_grid.read_grid(out)
    assert open(out).readline().startswith("# ") and len(back["auc"]) == 6
    for name in svm_grid.COLUMNS:
        assert np.array_equal(back[name], table[name], equal_nan=True), name
    assert back["best"] == table["best"] and np.isfinite(back["auc"]).all()
