"""
svm.py -- drop-in for the part of scikit-learn's ``svm`` module that PhaMers uses (scripts/phamer.py:258-266,
``from sklearn import svm``; ``svm.NuSVC()``): a binary Nu-SVC with an RBF kernel, fitted and evaluated on the GPU
(svm.cpp of scikit-learn's libsvm fork restated in svm.hip, without shrinking: it equals NuSVC(shrinking=False).
scikit-learn's default NuSVC() shrinks; that gives the same fit on the reference's data, but not on every input --
DESIGN.md section 4.7).

    NuSVC(nu=0.5, gamma='scale', tol=1e-3)      fit / predict / decision_function,
                                                support_, support_vectors_, dual_coef_, intercept_, n_iter_, classes_
    nusvc_sweep(X, y, nus, gammas, folds=None, seed=None)
                                                every NuSVC(nu, gamma) of a grid, with the fits of an N-fold split and their
                                                held-out decisions, side by side on the device (svm_sweep.hip)

The attributes follow scikit-learn's binary conventions: classes_ sorted, dual_coef_ and intercept_ the negated libsvm
values, decision_function > 0 for classes_[1], and predict gives classes_[1] where libsvm's value is <= 0.  Other kernels,
probability outputs, sample weights and more than two classes raise NotImplementedError.
"""
import numpy as np

from . import _lib

__all__ = ["NuSVC", "nusvc_sweep", "NuSVCSweep"]

# a sweep problem's status (PHK_SVM_*)
STATUS_OK, STATUS_INFEASIBLE, STATUS_NOT_FINITE = _lib.SVM_OK, _lib.SVM_INFEASIBLE, _lib.SVM_NOT_FINITE


class NuSVC(object):

    def __init__(self, nu=0.5, kernel='rbf', gamma='scale', tol=1e-3, shrinking=True, probability=False, max_iter=-1):
        if kernel != 'rbf':
            raise NotImplementedError("NuSVC: only kernel='rbf' runs on the GPU (got %r)" % (kernel,))
        if probability:
            raise NotImplementedError("NuSVC: probability=True is not supported")
        self.nu, self.kernel, self.gamma, self.tol = nu, kernel, gamma, tol
        self.shrinking = shrinking      # (accepted and ignored: the device solver never shrinks; see the module docstring)
        self.probability, self.max_iter = probability, max_iter

    def fit(self, X, y, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError("NuSVC: sample_weight is not supported")
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.asarray(y)
        if X.ndim != 2 or y.ndim != 1 or len(y) != len(X):
            raise ValueError("X must be 2-D and y 1-D with one label per row")
        if np.isnan(X).any():
            raise ValueError("Input contains NaN.")
        self.classes_, codes = np.unique(y, return_inverse=True)
        if len(self.classes_) < 2:
            raise ValueError("The number of classes has to be greater than one; got %d class" % len(self.classes_))
        if len(self.classes_) > 2:
            raise NotImplementedError("NuSVC: multi-class data is not supported")
        # svm_check_parameter (svm.cpp:3129), before any device work
        n1 = int(codes.sum())
        n0 = len(codes) - n1
        if not 0 < self.nu <= 1:
            raise ValueError("nu <= 0 or nu > 1")
        if self.nu * (n0 + n1) / 2 > min(n0, n1):
            raise ValueError("specified nu is infeasible")
        self._gamma = _lib.svm_gamma(X, self.gamma)
        support, coef, rho, n_iter = _lib.nusvc_fit(_lib.get_context(), X, codes.astype(np.float64), self.nu, self._gamma,
                                                    self.tol, self.max_iter)
        self.support_ = support
        self.support_vectors_ = X[support]
        self.n_support_ = np.array([int((codes[support] == 0).sum()), int((codes[support] == 1).sum())], dtype=np.int32)
        self._libsvm_coef, self._libsvm_rho = coef, rho
        self.dual_coef_ = -coef[None, :]
        self.intercept_ = np.array([rho])
        self.n_iter_ = np.array([n_iter], dtype=np.int32)
        self.shape_fit_ = X.shape
        return self

    def _libsvm_decision(self, X):
        if not hasattr(self, "support_"):
            raise ValueError("This NuSVC instance is not fitted yet. Call 'fit' first.")
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] != self.shape_fit_[1]:
            raise ValueError("X has %s features, but NuSVC is expecting %d" % (X.shape[1:], self.shape_fit_[1]))
        if np.isnan(X).any():
            raise ValueError("Input contains NaN.")
        return _lib.nusvc_decision(_lib.get_context(), self.support_vectors_, self._libsvm_coef, self._libsvm_rho,
                                   self._gamma, X)

    def decision_function(self, X):
        return -self._libsvm_decision(X)

    def predict(self, X):
        return self.classes_[np.where(self._libsvm_decision(X) <= 0, 1, 0)]


class NuSVCSweep(object):
    """What nusvc_sweep returns; the fields are listed there."""

    def cell(self, gamma_index, nu_index):
        """(gamma, nu) of a cell as numbers."""
        return float(self.gammas[gamma_index]), float(self.nus[nu_index])


def nusvc_sweep(X, y, nus, gammas, folds=None, seed=None, tol=1e-3, max_iter=-1, _lds_rows=-1, _gammas_per_pass=0, _threads=0):
    """``NuSVC(nu, gamma=g, tol=tol, max_iter=max_iter).fit(X, y)`` for every g of ``gammas`` and nu of ``nus`` -- and, with
    ``folds=N``, the same fit on the train rows of every fold of ``cross_validate.FoldPlan(n+, n-, N, seed)`` (class
    ``classes_[1]`` is "positive") with the decisions of the fold's held-out rows -- solved side by side: one workgroup per
    fit, one kernel matrix per gamma (phk_nusvc_sweep).  Every number is bit for bit what the single
    fit and its ``decision_function`` give.

    ``gammas`` are numbers; 'scale' / 'auto' are resolved ONCE over all rows (``_lib.svm_gamma``) and the same value serves
    every fold (``NuSVC`` on a fold's rows alone would take 'scale' over those rows).  Returns a ``NuSVCSweep`` with ``nus``
    (V,), ``gammas`` (Gm,), ``classes_`` and, per cell (g, v):
        status (Gm, V)            0, or the first non-zero status among the full fit and the folds: STATUS_INFEASIBLE (a class
                                  without rows or nu (n0 + n1) / 2 > min(n0, n1) -- where NuSVC.fit raises "infeasible" /
                                  "greater than one"), STATUS_NOT_FINITE (r = 0, where it raises "not finite")
        n_iter, n_support (Gm, V) int32, of the full fit
        intercept (Gm, V), dual_coef (Gm, V, n)   of the full fit in scikit-learn's sign, dual_coef dense in the row order of
                                  ``X``, 0 off the support
    and with folds also ``fold_of`` (n,), ``fold_status`` / ``fold_n_iter`` / ``fold_n_support`` / ``fold_intercept``
    (Gm, V, N) and ``fold_dual_coef`` (Gm, V, N, n) -- each fold's own fit, NaN where that fit has a status, 0 at its held-out
    rows --, ``held_decision`` (Gm, V, n) in ``decision_function``'s sign, ``held_predict`` (Gm, V, n): 1.0 where the row is
    predicted ``classes_[1]``, else 0.0, ``auc`` (Gm, V) -- ``learning.predictor_performance`` of the
    held-out decisions of class 1 against class 0 -- and ``accuracy`` (Gm, V).  A cell with a non-zero status carries NaN in
    its float fields; no cell raises.  ValueError, before any device work, for an empty axis, nu outside (0, 1], a gamma that
    is not finite and > 0, NaN rows or more or fewer than two classes.  The ``_`` arguments are for the tests (state in LDS
    up to that many rows, kernel matrices resident at a time, solver threads): no result depends on them."""
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("X must be 2-D and y 1-D with one label per row")
    classes, codes = np.unique(y, return_inverse=True)
    if len(classes) != 2:
        raise ValueError("The number of classes has to be two; got %d class(es)" % len(classes))
    X = np.ascontiguousarray(X, dtype=np.float64)
    glist = [gammas] if isinstance(gammas, str) or np.ndim(gammas) == 0 else list(gammas)
    if X.ndim != 2 or len(X) != len(y):
        raise ValueError("X must be 2-D and y 1-D with one label per row")
    if np.isnan(X).any():
        raise ValueError("Input contains NaN.")
    gvals = [_lib.svm_gamma(X, g) for g in glist]
    fold_of, N = None, 0
    if folds is not None:
        from . import cross_validate
        N = int(folds)
        if N < 1:
            raise ValueError("folds must be at least 1, got %r" % (folds,))
        plan = cross_validate.FoldPlan(int((codes == 1).sum()), int((codes == 0).sum()), N, seed)
        fold_of = np.empty(len(y), dtype=np.int32)
        fold_of[codes == 1], fold_of[codes == 0] = plan.positive, plan.negative
    X, lab, nus, gvals, fold_of = _lib.check_nusvc_sweep_arguments(X, codes, nus, gvals, fold_of, N, tol, max_iter)
    raw = _lib.nusvc_sweep(_lib.get_context(), X, lab, nus, gvals, fold_of, N, tol, max_iter, _lds_rows, _gammas_per_pass,
                           _threads)
    st = raw["status"]
    bad = st != 0
    cell_status = np.where(bad.any(axis=2), np.take_along_axis(st, bad.argmax(axis=2)[..., None], axis=2)[..., 0], 0)
    dead = cell_status != 0
    out = NuSVCSweep()
    out.nus, out.gammas, out.classes_ = nus, gvals, classes
    out.status = cell_status.astype(np.int32)
    out.n_iter, out.n_support = raw["n_iter"][:, :, 0].copy(), raw["n_sv"][:, :, 0].copy()
    out.intercept = np.where(dead, np.nan, raw["rho"][:, :, 0])
    out.dual_coef = np.where(dead[..., None], np.nan, -raw["coef"][:, :, 0, :])
    if N:
        out.fold_of = fold_of
        out.fold_status, out.fold_n_iter = st[:, :, 1:].copy(), raw["n_iter"][:, :, 1:].copy()
        out.fold_n_support, out.fold_intercept = raw["n_sv"][:, :, 1:].copy(), raw["rho"][:, :, 1:].copy()
        out.fold_dual_coef = np.where((out.fold_status != 0)[..., None], np.nan, -raw["coef"][:, :, 1:, :])
        dec = raw["held_dec"]
        out.held_decision = np.where(dead[..., None], np.nan, -dec)
        out.held_predict = np.where(dead[..., None], np.nan, np.where(dec <= 0, 1.0, 0.0))
        out.auc, out.accuracy = np.full(dead.shape, np.nan), np.full(dead.shape, np.nan)
        from . import learning
        for g, v in zip(*np.nonzero(~dead)):
            d = out.held_decision[g, v]
            out.auc[g, v] = learning.predictor_performance(d[codes == 1], d[codes == 0])[2]
            out.accuracy[g, v] = float((out.held_predict[g, v] == codes).mean())
    return out

