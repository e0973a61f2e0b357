"""
svm.py -- drop-in for the part of scikit-learn's ``svm`` module that PhaMers uses (scripts/phamer.py:258-266,
``from sklearn import svm``; ``svm.NuSVC()``): a binary Nu-SVC with an RBF kernel, fitted and evaluated on the GPU
(svm.cpp of scikit-learn's libsvm fork restated in svm.hip, without shrinking: it equals NuSVC(shrinking=False).
scikit-learn's default NuSVC() shrinks; that gives the same fit on the reference's data, but not on every input --
DESIGN.md section 4.7).

    NuSVC(nu=0.5, gamma='scale', tol=1e-3)      fit / predict / decision_function,
                                                support_, support_vectors_, dual_coef_, intercept_, n_iter_, classes_

The attributes follow scikit-learn's binary conventions: classes_ sorted, dual_coef_ and intercept_ the negated libsvm
values, decision_function > 0 for classes_[1], and predict gives classes_[1] where libsvm's value is <= 0.  Other kernels,
probability outputs, sample weights and more than two classes raise NotImplementedError.
"""
import numpy as np

from . import _lib

__all__ = ["NuSVC"]


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
