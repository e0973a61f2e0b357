"""The NuSVC nu x gamma sweep restated as a loop over tests/svm_ref.Fit (test-only): one fit on all rows per cell and one per
fold of cross_validate.FoldPlan(n+, n-, N, seed), class 1 "positive", with the held-out decisions of each fold's fit."""
import numpy as np

from tests import svm_ref

OK, INFEASIBLE, NOT_FINITE = 0, 1, 2


def fold_ids(y, folds, seed):
    """fold_of (n,) as svm.nusvc_sweep assigns it: FoldPlan's positive assignment over the rows of class 1 in order, its
    negative assignment over the rows of class 0."""
    from phamers_amd import cross_validate
    y = np.asarray(y)
    plan = cross_validate.FoldPlan(int((y == 1).sum()), int((y == 0).sum()), folds, seed)
    out = np.empty(len(y), dtype=np.int32)
    out[y == 1], out[y == 0] = plan.positive, plan.negative
    return out


def fit_or_status(fit, X, y, nu, gamma, tol=1e-3, max_iter=-1):
    """(fit, OK), or (None, status) where the fit raises as libsvm / scikit-learn do.  ``fit(X, y, nu, gamma, tol, max_iter)``
    returns an object with support_, dual_coef_, intercept_, n_iter_ and decision_function."""
    try:
        return fit(X, y, nu, gamma, tol, max_iter), OK
    except ValueError as e:
        msg = str(e)
        if "infeasible" in msg or "greater than one" in msg:
            return None, INFEASIBLE
        if "not finite" in msg:
            return None, NOT_FINITE
        raise


def ref_fit(X, y, nu, gamma, tol, max_iter):
    return svm_ref.Fit(X, y, nu=nu, gamma=gamma, tol=tol, max_iter=max_iter)


def sweep(X, y, nus, gammas, folds=None, seed=None, tol=1e-3, max_iter=-1, fit=ref_fit):
    """{(g, v): cell} with cell = {"full": (fit, status), "folds": [(fit, status, held mask)], "held_decision": (n,) or None}
    for gamma index g and nu index v; ``gammas`` are numbers."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    fold_of = fold_ids(y, folds, seed) if folds else None
    out = {}
    for g, gamma in enumerate(gammas):
        for v, nu in enumerate(nus):
            cell = {"full": fit_or_status(fit, X, y, nu, gamma, tol, max_iter), "folds": [], "held_decision": None}
            if folds:
                dec = np.full(len(y), np.nan)
                for f in range(folds):
                    held = fold_of == f
                    m, st = fit_or_status(fit, X[~held], y[~held], nu, gamma, tol, max_iter)
                    cell["folds"].append((m, st, held))
                    if m is not None and held.any():
                        dec[held] = m.decision_function(X[held])
                cell["held_decision"] = dec
            out[(g, v)] = cell
    return out


def dense_coef(m, n, rows=None):
    """dual_coef_ of a fit as a dense (n,) vector over the caller's rows (``rows``: the fit's rows among them)."""
    out = np.zeros(n)
    sup = m.support_ if rows is None else np.flatnonzero(rows)[m.support_]
    out[sup] = m.dual_coef_[0]
    return out
