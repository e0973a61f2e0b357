"""CPU: the restatement of the NuSVC nu x gamma sweep (tests/svm_sweep_ref.py) against scikit-learn, and the host-side rules
of svm.nusvc_sweep and phamers_amd.svm_grid -- argument checks, the CSV, the command line's defaults, the scorer's and the
validator's new attributes -- without a device."""
import numpy as np
import pytest

from tests import svm_sweep_ref
from tests.test_svm_host import EXACT

NUS, GAMMAS, FOLDS, SEED = (0.2, 0.4, 0.6), (0.5, 2.0, 8.0), 3, 4


def _dyadic():
    rng = np.random.default_rng(11)
    X = rng.integers(0, 8, (120, 9)) / 8.0
    y = (X[:, 0] + X[:, 1] + 0.5 * rng.random(120) > 1.1).astype(np.float64)
    return X, y


def test_restated_sweep_equals_scikit_learn_on_a_grid():
    """The loop over svm_ref.Fit with the FoldPlan split against NuSVC(nu, gamma=g, shrinking=False) on a 3 x 3 grid of
    120 x 9 dyadic rows with 3 folds: the same iterations and support, coefficients and intercept within 1e-12, for the fit
    on all rows and for every fold's fit; the infeasible fits are the ones scikit-learn refuses."""
    from sklearn.svm import NuSVC

    def skl_fit(X, y, nu, gamma, tol, max_iter):
        return NuSVC(nu=nu, gamma=gamma, tol=tol, max_iter=max_iter, shrinking=False).fit(X, y)

    X, y = _dyadic()
    assert 30 < y.sum() < 90
    ours = svm_sweep_ref.sweep(X, y, NUS, GAMMAS, FOLDS, SEED)
    theirs = svm_sweep_ref.sweep(X, y, NUS, GAMMAS, FOLDS, SEED, fit=skl_fit)
    fits = 0
    for key, cell in ours.items():
        other = theirs[key]
        pairs = [(cell["full"], other["full"])] + [(a[:2], b[:2]) for a, b in zip(cell["folds"], other["folds"])]
        assert len(pairs) == FOLDS + 1
        for (m, st), (w, wst) in pairs:
            assert st == wst, key
            if m is None:
                continue
            fits += 1
            assert int(m.n_iter_[0]) == int(w.n_iter_[0]), key
            assert np.array_equal(m.support_, w.support_), key
            assert np.max(np.abs(m.dual_coef_[0] - w.dual_coef_[0])) <= EXACT, key
            assert abs(m.intercept_[0] - w.intercept_[0]) <= EXACT, key
        assert np.allclose(cell["held_decision"], other["held_decision"], rtol=0, atol=1e-9, equal_nan=True), key
    assert fits >= 24


def test_fold_ids_follow_the_validators_plan():
    from phamers_amd import cross_validate
    y = np.array([1, 0, 0, 1, 1, 0, 1, 0, 0, 0], dtype=np.float64)
    got = svm_sweep_ref.fold_ids(y, 3, 7)
    plan = cross_validate.FoldPlan(4, 6, 3, 7)
    assert np.array_equal(got[y == 1], plan.positive) and np.array_equal(got[y == 0], plan.negative)


def test_sweep_arguments_are_checked_before_any_device_work():
    from phamers_amd import _lib, svm
    X, y = _dyadic()
    for nus, gammas in (([], [1.0]), ([0.5], [])):
        with pytest.raises(ValueError, match="empty axis"):
            svm.nusvc_sweep(X, y, nus, gammas)
    for nu in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="nu <= 0 or nu > 1"):
            svm.nusvc_sweep(X, y, [0.5, nu], [1.0])
    for gamma in (0.0, -1.0, float("inf"), float("nan"), "other"):
        with pytest.raises(ValueError, match="gamma"):
            svm.nusvc_sweep(X, y, [0.5], [1.0, gamma])
    with pytest.raises(ValueError, match="NaN"):
        Xn = X.copy()
        Xn[5, 2] = np.nan
        svm.nusvc_sweep(Xn, y, [0.5], [1.0])
    with pytest.raises(ValueError, match="classes"):
        svm.nusvc_sweep(X, np.ones(len(y)), [0.5], [1.0])
    with pytest.raises(ValueError, match="classes"):
        svm.nusvc_sweep(X, np.arange(len(y)) % 3, [0.5], [1.0])
    with pytest.raises(ValueError, match="one label per row"):
        svm.nusvc_sweep(X, y[:-1], [0.5], [1.0])
    with pytest.raises(ValueError, match="folds"):
        svm.nusvc_sweep(X, y, [0.5], [1.0], folds=0)
    with pytest.raises(ValueError, match="tol"):
        svm.nusvc_sweep(X, y, [0.5], [1.0], tol=0.0)
    with pytest.raises(ValueError, match="max_iter"):
        svm.nusvc_sweep(X, y, [0.5], [1.0], max_iter=0)
    # the binding's own check: fold ids and labels
    ok = _lib.check_nusvc_sweep_arguments(X, y, [0.5], [1.0], np.arange(len(y)) % 3, 3, 1e-3, -1)
    assert ok[4].dtype == np.int32 and ok[2].dtype == np.float64
    with pytest.raises(ValueError, match="fold id"):
        _lib.check_nusvc_sweep_arguments(X, y, [0.5], [1.0], np.arange(len(y)) % 4, 3, 1e-3, -1)
    with pytest.raises(ValueError, match="labels"):
        _lib.check_nusvc_sweep_arguments(X, y + 1, [0.5], [1.0], None, 0, 1e-3, -1)
    assert _lib.nusvc_sweep_lds_rows() == (160 * 1024 - 1024) // 17


def test_grid_csv_round_trip(tmp_path):
    from phamers_amd import svm_grid
    table = {"gamma": np.array([0.1, 0.1, 554.7712345678901]), "nu": np.array([0.25, 0.5, 1 / 3]),
             "n_support": np.array([12.0, 2358.0, 7.0]), "n_iter": np.array([3.0, 1278.0, 0.0]),
             "auc": np.array([0.5, 0.987654321012345, np.nan]), "accuracy": np.array([2 / 3, 0.9, np.nan])}
    path = str(tmp_path / "grid.csv")
    svm_grid.save_grid(path, table, args=svm_grid._parser().parse_args(["--nu", "0.5", "--gamma", "1", "-N", "5"]))
    lines = open(path).read().splitlines()
    assert lines[0].startswith("# ") and "gamma,nu,n_support,n_iter,auc,accuracy" in lines[0]
    assert all(line.startswith("# ") for line in lines[:-3]) and lines[-2] == "0.1,0.5,2358,1278,0.987654321012345,0.9"
    back = svm_grid.read_grid(path)
    for name in svm_grid.COLUMNS:
        assert np.array_equal(back[name], table[name], equal_nan=True), name
    assert back["best"] == 1
    svm_grid.save_grid(path, {k: v[2:] for k, v in table.items()})
    assert svm_grid.read_grid(path)["best"] is None


def test_grid_command_line_defaults():
    from phamers_amd import svm_grid
    a = svm_grid._parser().parse_args(["-pf", "p.csv", "-nf", "n.csv", "--nu", "0.25", "0.5", "--gamma", "1", "10", "-N", "5"])
    assert (a.nu, a.gamma, a.gamma_scale, a.N_fold, a.seed, a.output_file) == ([0.25, 0.5], [1.0, 10.0], [], 5, None, None)
    assert (a.positive_features_file, a.negative_features_file, a.data_directory) == ("p.csv", "n.csv", None)
    b = svm_grid._parser().parse_args(["-data", "d", "--nu", "0.5", "--gamma_scale", "0.25", "4", "-N", "3", "--seed", "2",
                                       "-out", "t.csv"])
    assert (b.gamma, b.gamma_scale, b.seed, b.output_file, b.data_directory) == ([], [0.25, 4.0], 2, "t.csv", "d")
    for argv in (["--gamma", "1", "-N", "5"], ["--nu", "0.5", "--gamma", "1"]):      # --nu and -N are required
        with pytest.raises(SystemExit):
            svm_grid._parser().parse_args(argv)
    with pytest.raises(SystemExit):                                                     # a gamma axis is required
        svm_grid.main(["-pf", "p.csv", "-nf", "n.csv", "--nu", "0.5", "-N", "5"])
    with pytest.raises(ValueError, match="folds"):
        svm_grid.grid(np.zeros((4, 2)), np.ones((4, 2)), [0.5], [1.0], folds=1)


def test_scorer_and_validator_carry_the_defaults_of_nusvc():
    from phamers_amd import cross_validate, phamer
    for obj in (phamer.phamer_scorer(), cross_validate.cross_validator()):
        assert obj.svm_nu == 0.5 and obj.svm_gamma == 'scale'
