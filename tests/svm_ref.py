"""NumPy restatement of scikit-learn's NuSVC (RBF kernel, binary labels) for the svm scoring method (test-only).

It follows scikit-learn's libsvm fork (sklearn/svm/src/libsvm/svm.cpp, scikit-learn 1.7.2) without shrinking, i.e.
NuSVC(shrinking=False).  On the reference's data the default NuSVC() (shrinking on) takes the same iterations to the
same solution, but not in general (tests/golden/scoring_svm_synth.npz, case "shrink"):
    svm_group_classes (:2243)      rows grouped by sorted label: label-0 rows first (y = +1), then label-1 rows (y = -1)
    solve_nu_svc (:1646)           alpha filled class by class up to nu * l / 2; final scaling by 1 / r
    SVC_Q::get_Q (:1436)           Q_ij = (float)(y_i y_j K_ij)  (typedef float Qfloat, :79); QD_ii = 1
    Solver::Solve (:684-895)       gradient start, the two-variable update, G += Q_i d_i + Q_j d_j
    Solver_NU::select_working_set  (:1186) Gmax ties to the last index (>=), obj_diff <= obj_diff_min (last index)
    Solver_NU::calculate_rho (:1370)
    svm_check_parameter (:3129)    nu feasibility
Prediction uses k_function's direct differences (:452); scikit-learn's binary decision_function is the negated libsvm
value, and predict gives classes_[1] iff the libsvm value is <= 0.
"""
import numpy as np

TAU = 1e-12


def gamma_scale(X):
    """gamma='scale' as scikit-learn computes it (sklearn/svm/_base.py): 1 / (D * X.var()), 1.0 for zero variance."""
    X = np.asarray(X, dtype=np.float64)
    X_var = X.var()
    return 1.0 / (X.shape[1] * X_var) if X_var != 0 else 1.0


def check_nu(nu, n0, n1):
    """svm_check_parameter (svm.cpp:3129): the message libsvm returns, or None."""
    if nu <= 0 or nu > 1:
        return "nu <= 0 or nu > 1"
    if nu * (n0 + n1) / 2 > min(n0, n1):
        return "specified nu is infeasible"
    return None


def grouped_order(labels):
    """libsvm's row order after svm_group_classes for labels in {0, 1}: (perm, y) with y = +1 for label 0."""
    labels = np.asarray(labels)
    perm = np.concatenate((np.flatnonzero(labels == 0), np.flatnonzero(labels == 1)))
    y = np.where(labels[perm] == 0, 1, -1).astype(np.int8)
    return perm, y


def kernel_matrix(Xg, y, gamma):
    """Q[i][j] = (float32)(y_i y_j exp(-gamma (|x_i|^2 + |x_j|^2 - 2 x_i.x_j))) in float64 storage."""
    sq = np.einsum("ij,ij->i", Xg, Xg)
    K = np.exp(-gamma * (sq[:, None] + sq[None, :] - 2.0 * (Xg @ Xg.T)))
    Q = (y[:, None] * y[None, :] * K).astype(np.float32).astype(np.float64)
    np.fill_diagonal(Q, 1.0)
    return Q


def solve_nu(Q, y, nu, eps=1e-3, max_iter=-1, counters=None):
    """Solver_NU on the grouped problem with C = 1: (alpha, G, rho, r, n_iter) before the 1/r scaling.

    ``counters`` (a dict, optional) counts the TAU branches (quad_coef <= 0 replaced by TAU): "tau_j", candidates j of the
    working-set choice that were scored with TAU; "tau_same" / "tau_opposite", updates of a pair with the same / opposite
    y that used TAU.  (Solver_NU's pair always shares y -- i is the i candidate of j's class -- so "tau_opposite" stays
    0; the branch is libsvm's, kept as it is.)"""
    if counters is not None:
        for k in ("tau_j", "tau_same", "tau_opposite"):
            counters.setdefault(k, 0)
    l = len(y)
    pos = y == 1
    alpha = np.zeros(l)
    nu_l = 0.0                              # (accumulated as l additions of nu * C_i, C_i = 1)
    for _ in range(l):
        nu_l += nu * 1.0
    sum_pos = sum_neg = nu_l / 2
    for i in range(l):
        if y[i] == 1:
            alpha[i] = min(1.0, sum_pos)
            sum_pos -= alpha[i]
        else:
            alpha[i] = min(1.0, sum_neg)
            sum_neg -= alpha[i]
    G = np.zeros(l)
    for i in np.flatnonzero(alpha > 0):     # Solver::Solve, gradient start, rows in order
        G += alpha[i] * Q[i]
    it = 0
    while max_iter == -1 or it < max_iter:
        upper, lower = alpha >= 1.0, alpha <= 0.0
        # i candidates: -G (y = +1, not upper), G (y = -1, not lower); ties to the last index
        cp = np.flatnonzero(pos & ~upper)
        cn = np.flatnonzero(~pos & ~lower)
        Gmaxp, ip = -np.inf, -1
        if len(cp):
            v = -G[cp]
            Gmaxp = v.max()
            ip = cp[np.flatnonzero(v == Gmaxp)[-1]]
        Gmaxn, inn = -np.inf, -1
        if len(cn):
            v = G[cn]
            Gmaxn = v.max()
            inn = cn[np.flatnonzero(v == Gmaxn)[-1]]
        jp = np.flatnonzero(pos & ~lower)
        jn = np.flatnonzero(~pos & ~upper)
        Gmaxp2 = G[jp].max() if len(jp) else -np.inf
        Gmaxn2 = (-G[jn]).max() if len(jn) else -np.inf
        obj = np.full(l, np.inf)
        if ip != -1 and len(jp):
            gd = Gmaxp + G[jp]
            qc = 1.0 + 1.0 - 2.0 * Q[ip, jp]
            od = -(gd * gd) / np.where(qc > 0, qc, TAU)
            obj[jp] = np.where(gd > 0, od, np.inf)
            if counters is not None:
                counters["tau_j"] += int(((gd > 0) & ~(qc > 0)).sum())
        if inn != -1 and len(jn):
            gd = Gmaxn - G[jn]
            qc = 1.0 + 1.0 - 2.0 * Q[inn, jn]
            od = -(gd * gd) / np.where(qc > 0, qc, TAU)
            obj[jn] = np.where(gd > 0, od, np.inf)
            if counters is not None:
                counters["tau_j"] += int(((gd > 0) & ~(qc > 0)).sum())
        ok = np.isfinite(obj)
        if max(Gmaxp + Gmaxp2, Gmaxn + Gmaxn2) < eps or not ok.any():
            break
        m = obj[ok].min()
        j = np.flatnonzero(ok & (obj == m))[-1]
        i = ip if y[j] == 1 else inn
        it += 1
        ai, aj = alpha[i], alpha[j]
        Qij = Q[i, j]
        if y[i] != y[j]:
            qc = 1.0 + 1.0 + 2.0 * Qij
            if qc <= 0:
                qc = TAU
                if counters is not None:
                    counters["tau_opposite"] += 1
            delta = (-G[i] - G[j]) / qc
            diff = alpha[i] - alpha[j]
            alpha[i] += delta
            alpha[j] += delta
            if diff > 0:
                if alpha[j] < 0:
                    alpha[j], alpha[i] = 0.0, diff
            elif alpha[i] < 0:
                alpha[i], alpha[j] = 0.0, -diff
            if diff > 0.0:          # C_i - C_j = 0
                if alpha[i] > 1.0:
                    alpha[i], alpha[j] = 1.0, 1.0 - diff
            elif alpha[j] > 1.0:
                alpha[j], alpha[i] = 1.0, 1.0 + diff
        else:
            qc = 1.0 + 1.0 - 2.0 * Qij
            if qc <= 0:
                qc = TAU
                if counters is not None:
                    counters["tau_same"] += 1
            delta = (G[i] - G[j]) / qc
            s = alpha[i] + alpha[j]
            alpha[i] -= delta
            alpha[j] += delta
            if s > 1.0:
                if alpha[i] > 1.0:
                    alpha[i], alpha[j] = 1.0, s - 1.0
            elif alpha[j] < 0:
                alpha[j], alpha[i] = 0.0, s
            if s > 1.0:
                if alpha[j] > 1.0:
                    alpha[j], alpha[i] = 1.0, s - 1.0
            elif alpha[i] < 0:
                alpha[i], alpha[j] = 0.0, s
        di, dj = alpha[i] - ai, alpha[j] - aj
        G += Q[i] * di + Q[j] * dj
    rho, r = calculate_rho(alpha, G, y)
    return alpha, G, rho, r, it


def calculate_rho(alpha, G, y):
    """Solver_NU::calculate_rho (svm.cpp:1370): (rho, r) before the 1/r scaling; sums in row order."""
    out = []
    for cls in (1, -1):
        sel = y == cls
        a, g = alpha[sel], G[sel]
        up, lo = a >= 1.0, a <= 0.0
        free = ~up & ~lo
        if free.any():
            s = 0.0
            for v in g[free]:
                s += v
            out.append(s / free.sum())
        else:
            ub = g[lo].min() if lo.any() else np.inf
            lb = g[up].max() if up.any() else -np.inf
            out.append((ub + lb) / 2)
    r1, r2 = out
    return (r1 - r2) / 2, (r1 + r2) / 2


class Fit(object):
    """A fitted binary NuSVC in scikit-learn's terms: support_, dual_coef_ (1, n_SV), intercept_ (1,), n_iter_,
    _gamma, plus support_vectors_.  ``max_iter`` as NuSVC's (-1: no limit); ``counters`` as solve_nu's."""

    def __init__(self, X, labels, nu=0.5, gamma='scale', tol=1e-3, max_iter=-1, counters=None):
        X = np.asarray(X, dtype=np.float64)
        labels = np.asarray(labels)
        n1 = int((labels == 1).sum())
        n0 = len(labels) - n1
        if n0 == 0 or n1 == 0:
            raise ValueError("The number of classes has to be greater than one; got 1 class")
        msg = check_nu(nu, n0, n1)
        if msg:
            raise ValueError(msg)
        self._gamma = gamma_scale(X) if gamma == 'scale' else (1.0 / X.shape[1] if gamma == 'auto' else float(gamma))
        perm, y = grouped_order(labels)
        Q = kernel_matrix(X[perm], y, self._gamma)
        alpha, _, rho, r, it = solve_nu(Q, y, nu, tol, max_iter, counters)
        with np.errstate(divide="ignore", invalid="ignore"):
            coef = alpha * (y / r)            # solve_nu_svc: alpha[i] *= y[i] / r
            rho = rho / r
        sv = np.flatnonzero(alpha != 0)
        if not (np.isfinite(coef[sv]).all() and np.isfinite(rho)):     # sklearn/svm/_base.py, fit (r = 0)
            raise ValueError("The dual coefficients or intercepts are not finite. The input data may contain large values "
                             "and need to be preprocessed.")
        self.support_ = perm[sv].astype(np.int32)
        self.support_vectors_ = X[self.support_]
        self.dual_coef_ = -coef[sv][None, :]  # binary: scikit-learn negates libsvm's coefficients and rho
        self.intercept_ = np.array([rho])
        self.n_iter_ = np.array([it], dtype=np.int32)
        self.libsvm_coef = coef[sv]
        self.libsvm_rho = rho

    def libsvm_decision(self, Q):
        """libsvm's value: sum_sv coef_sv exp(-gamma |q - x_sv|^2) - rho, direct differences."""
        Q = np.asarray(Q, dtype=np.float64)
        out = np.empty(len(Q))
        for s in range(0, len(Q), 256):
            d = Q[s:s + 256, None, :] - self.support_vectors_[None, :, :]
            k = np.exp(-self._gamma * np.einsum("qsd,qsd->qs", d, d))
            out[s:s + 256] = k @ self.libsvm_coef - self.libsvm_rho
        return out

    def decision_function(self, Q):
        return -self.libsvm_decision(Q)

    def predict(self, Q):
        return np.where(self.libsvm_decision(Q) <= 0, 1.0, 0.0)


def decision(Q, SV, libsvm_coef, libsvm_rho, gamma):
    """libsvm's decision values for given support vectors / coefficients (direct differences)."""
    f = Fit.__new__(Fit)
    f.support_vectors_, f.libsvm_coef, f.libsvm_rho, f._gamma = np.asarray(SV, np.float64), np.asarray(libsvm_coef), \
        float(libsvm_rho), float(gamma)
    return f.libsvm_decision(Q)
