"""NumPy restatement of the k-means sweep (test-only), float64 direct differences throughout: scikit-learn's k-means++
seeding with its closest call (the seeding margin of DESIGN.md 4.9), its Lloyd iteration with the smallest relative
assignment gap over all sweeps, and silhouettes.  Used by tools/gen_golden_sweep.py and the sweep's tests."""
import numpy as np

from tests import cluster_ref


def draws(n, k, seed):
    """The random draws of scikit-learn's k-means++ from a fresh RandomState(seed): (first row, uniforms (k - 1, T))."""
    rs = np.random.RandomState(seed)
    w = np.ones(n, dtype=np.float64)
    first = int(rs.choice(n, p=w / w.sum()))
    T = 2 + int(np.log(k))
    return first, np.array([rs.uniform(size=T) for _ in range(1, k)], dtype=np.float64).reshape(k - 1, T)


def sq_dists(A, X, rows=64):
    """(len(A), len(X)) squared direct-difference distances."""
    A = np.asarray(A, dtype=np.float64)
    out = np.empty((A.shape[0], X.shape[0]))
    for s in range(0, X.shape[0], rows):
        out[:, s:s + rows] = ((X[None, s:s + rows, :] - A[:, None, :]) ** 2).sum(axis=2)
    return out


def centre(X):
    X = np.array(X, dtype=np.float64, order="C")
    X -= X.mean(axis=0)
    return X


def kmeans_plusplus(Xc, k, seed):
    """(chosen rows (k,), margin): scikit-learn's _kmeans_plusplus on the centred rows ``Xc`` -- one trial row per draw by
    searchsorted on the cumulative closest distances, the trial with the smallest potential wins (first on ties) -- and the
    closest call of the fit, relative to the potential: a draw's distance to the nearer of the two cumulative values
    around it; the gap between the best trial's potential and the best trial on another row.  A draw past the total and a
    zero potential with centres still to come count as margin 0."""
    n = Xc.shape[0]
    first, u = draws(n, k, seed)
    idx = np.empty(k, dtype=np.int64)
    idx[0] = first
    closest = sq_dists(Xc[first:first + 1], Xc)[0]
    pot = closest.sum()
    margin = np.inf
    if k > 1 and not pot > 0:
        margin = 0.0
    for c in range(1, k):
        vals = u[c - 1] * pot
        cum = np.cumsum(closest)
        cand = np.searchsorted(cum, vals)
        for t, v in zip(cand, vals):
            if t >= n or not pot > 0:
                margin = 0.0
            else:
                margin = min(margin, min(cum[t] - v, v - (cum[t - 1] if t else 0.0)) / pot)
        cand = np.clip(cand, None, n - 1)
        d = np.minimum(closest, sq_dists(Xc[cand], Xc))
        pots = d.sum(axis=1)
        best = int(np.argmin(pots))
        for t in range(len(cand)):
            if cand[t] != cand[best]:
                g = (pots[t] - pots[best]) / pots[best] if pots[best] > 0 else 0.0
                margin = min(margin, g)
        pot = pots[best]
        closest = d[best]
        idx[c] = cand[best]
        if c + 1 < k and not pot > 0:
            margin = 0.0
    return idx, float(margin)


def lloyd(Xc, init_rows, tol=1e-4, max_iter=300):
    """scikit-learn's _kmeans_single_lloyd from the given rows as centres: (labels, sweeps, smallest relative gap between a
    point's two nearest centres over all E-steps, empty clusters met).  Ties to the lower centre; an empty cluster keeps
    its centre (scikit-learn relocates it: such a fit is not comparable)."""
    n, k = Xc.shape[0], len(init_rows)
    tol_abs = float(np.mean(np.var(Xc, axis=0)) * tol)
    cen = Xc[np.asarray(init_rows)].copy()
    labels = np.full(n, -1, dtype=np.int64)
    gap, empties, strict, it = np.inf, 0, False, 0

    def e_step():
        d = sq_dists(cen, Xc).T                       # (n, k)
        lab = np.argmin(d, axis=1)
        g = np.inf
        if k > 1:
            part = np.partition(d, 1, axis=1)
            best, second = part[:, 0], part[:, 1]
            ok = (second > 0) & np.isfinite(second)
            if ok.any():
                g = float(((second[ok] - best[ok]) / second[ok]).min())
        return lab, g

    for it in range(1, max_iter + 1):
        lab, g = e_step()
        gap = min(gap, g)
        new = cen.copy()
        for c in range(k):
            m = lab == c
            if m.any():
                new[c] = Xc[m].sum(axis=0) / m.sum()
            else:
                empties += 1
        shift = float(((new - cen) ** 2).sum())
        changed = not np.array_equal(lab, labels)
        labels, cen = lab, new
        if not changed:
            strict = True
            break
        if shift <= tol_abs:
            break
    if not strict:
        labels, g = e_step()
        gap = min(gap, g)
    return labels.astype(np.int32), it, float(gap), empties


def kmeans(X, k, seed=10, tol=1e-4, max_iter=300):
    """dict(labels, n_iter, seeds, seed_margin, min_gap, n_empty) of KMeans(k, random_state=seed).fit(X), restated."""
    Xc = centre(X)
    rows, margin = kmeans_plusplus(Xc, int(k), seed)
    labels, n_iter, gap, empties = lloyd(Xc, rows, tol, max_iter)
    return {"labels": labels, "n_iter": n_iter, "seeds": rows, "seed_margin": margin, "min_gap": gap, "n_empty": empties}


def silhouettes(X, labels):
    """silhouette_samples with direct-difference distances (cluster_ref's)."""
    return cluster_ref.silhouettes(X, labels)
