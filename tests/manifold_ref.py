"""NumPy float64 restatement of every stage of phamers_amd.manifold and of the descent loop (test-only), the counterpart of
cluster_ref.py / density_ref.py.  tests/test_manifold_host.py holds it to scikit-learn; tests/test_gpu_manifold.py holds
the device to it."""
import numpy as np

MACHINE_EPSILON = np.finfo(np.double).eps


# ---- fused multiply-add, exactly (Boldo & Melquiond, "Emulation of FMA and correctly rounded sums", 2008) ----------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    c = 134217729.0   # 2^27 + 1 (Veltkamp split)
    ta, tb = c * a, c * b
    ah = ta - (ta - a)
    bh = tb - (tb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_round_to_odd(a, b):
    s, e = _two_sum(a, b)
    bits = s.view(np.int64)
    fix = (e != 0.0) & ((bits & 1) == 0)
    # move one ulp towards the error: for s > 0 up when e > 0, down when e < 0 (mirrored for s < 0); either makes it odd
    step = np.where((e > 0) == (s > 0), 1, -1)
    return np.where(fix, (bits + step).view(np.float64), s)


def fma(a, b, c):
    """round(a * b + c) with one rounding, elementwise (no overflow / underflow in the test data)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    a, b, c = a.copy(), b.copy(), c.copy()
    ph, pl = _two_prod(a, b)
    uh, ul = _two_sum(c, ph)
    return uh + _add_round_to_odd(pl, ul)


# ---- PCA ---------------------------------------------------------------------------------------------------------------
def pca(X, n_components):
    """(transformed, components, mean, explained_variance): eigh of the centred covariance, largest-|.| entry of each
    component positive."""
    X = np.asarray(X, np.float64)
    mean = X.mean(axis=0)
    Xc = X - mean
    w, v = np.linalg.eigh(Xc.T @ Xc / (X.shape[0] - 1))
    order = np.argsort(-w, kind="stable")[:n_components]
    comps = v[:, order].T.copy()
    big = np.argmax(np.abs(comps), axis=1)
    comps *= np.sign(comps[np.arange(n_components), big])[:, None]
    return Xc @ comps.T, comps, mean, w[order]


# ---- neighbour graph ---------------------------------------------------------------------------------------------------
def sqdist_rows(Z, rows):
    """(len(rows), n) squared distances of the given rows to every row: direct differences accumulated by fma in column
    order, the device's form."""
    Z = np.asarray(Z, np.float64)
    s = np.zeros((len(rows), Z.shape[0]))
    for c in range(Z.shape[1]):
        d = Z[rows, c][:, None] - Z[None, :, c]
        s = fma(d, d, s)
    return s


def neighbors(Z, k, rows=None):
    """(indices, squared distances) of the k nearest other rows of the given rows (all by default), by (distance, index)."""
    Z = np.asarray(Z, np.float64)
    rows = np.arange(Z.shape[0]) if rows is None else np.asarray(rows)
    idx = np.empty((len(rows), k), np.int32)
    d2 = np.empty((len(rows), k))
    for s in range(0, len(rows), 256):
        r = rows[s:s + 256]
        D = sqdist_rows(Z, r)
        D[np.arange(len(r)), r] = np.inf
        for a in range(len(r)):
            o = np.lexsort((np.arange(Z.shape[0]), D[a]))[:k]
            idx[s + a], d2[s + a] = o, D[a, o]
    return idx, d2


def kth_gap(Z, k):
    """min over rows of (d_(k+1) - d_k) / d_(k+1) between DIFFERENT squared distances at the neighbourhood's edge (inf when
    there is no (k+1)-th neighbour): the generator refuses inputs where it is below 1e-9."""
    Z = np.asarray(Z, np.float64)
    if k + 1 > Z.shape[0] - 1:
        return np.inf
    sq = (Z ** 2).sum(axis=1)
    a, b = np.empty(Z.shape[0]), np.empty(Z.shape[0])
    for s in range(0, Z.shape[0], 1024):   # (plain distances: a margin of 1e-9 does not need the device's bits)
        D = np.maximum(sq[s:s + 1024, None] + sq[None, :] - 2.0 * Z[s:s + 1024] @ Z.T, 0.0)
        D[np.arange(D.shape[0]), np.arange(s, s + D.shape[0])] = np.inf
        part = np.partition(D, (k - 1, k), axis=1)
        a[s:s + 1024], b[s:s + 1024] = part[:, k - 1], part[:, k]
    b = np.where(np.abs(b - a) <= 1e-12 * np.abs(b), a, b)   # the same distance up to the Gram form's rounding: a tie
    rel = np.where(b > a, (b - a) / np.where(b > 0, b, 1.0), np.inf)
    return float(rel.min())


# ---- affinities --------------------------------------------------------------------------------------------------------
def binary_search_perplexity(d2, perplexity):
    """sklearn/manifold/_utils.pyx _binary_search_perplexity on float64 squared distances: (P, beta).  The target is
    log(float32(perplexity)), scikit-learn's argument being a C float."""
    d2 = np.asarray(d2, np.float64)
    n, k = d2.shape
    target = np.log(float(np.float32(perplexity)))
    P = np.zeros((n, k))
    beta_out = np.empty(n)
    for i in range(n):
        d = d2[i]
        beta, bmin, bmax = 1.0, -np.inf, np.inf
        for _ in range(100):
            p = np.exp(-d * beta)
            sum_p = float(np.cumsum(p)[-1])
            if sum_p == 0.0:
                sum_p = 1e-8
            p = p / sum_p
            H = np.log(sum_p) + beta * float(np.cumsum(d * p)[-1])
            diff = H - target
            if abs(diff) <= 1e-5:
                break
            if diff > 0.0:
                bmin = beta
                beta = beta * 2.0 if bmax == np.inf else (beta + bmax) / 2.0
            else:
                bmax = beta
                beta = beta / 2.0 if bmin == -np.inf else (beta + bmin) / 2.0
        P[i], beta_out[i] = p, beta
    return P, beta_out


def symmetrize(idx, P):
    """(P + P.T) / sum as CSR (indptr, indices, values), columns ascending within a row."""
    idx = np.asarray(idx, np.int64)
    n, k = idx.shape
    src = np.repeat(np.arange(n, dtype=np.int64), k)
    dst = idx.ravel()
    key = np.concatenate((src * n + dst, dst * n + src))
    val = np.concatenate((P.ravel(), P.ravel()))
    o = np.argsort(key, kind="stable")
    key, val = key[o], val[o]
    first = np.concatenate(([True], key[1:] != key[:-1]))
    starts = np.flatnonzero(first)
    values = np.add.reduceat(val, starts)
    ukey = key[starts]
    rows, cols = ukey // n, (ukey % n).astype(np.int32)
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, rows + 1, 1)
    indptr = np.cumsum(indptr)
    total = max(float(np.cumsum(values)[-1]), MACHINE_EPSILON)
    return indptr, cols, values / total


def dense(csr):
    indptr, cols, vals = csr
    n = len(indptr) - 1
    out = np.zeros((n, n))
    out[np.repeat(np.arange(n), np.diff(indptr)), cols] = vals
    return out


# ---- objective, gradient, descent --------------------------------------------------------------------------------------
def kl_gradient(Y, csr, exaggeration=1.0, rows=None):
    """(KL, grad) as phk_tsne_gradient defines them; ``rows``: the gradient of those rows only (Z and KL stay whole)."""
    indptr, cols, vals = csr
    Y = np.asarray(Y, np.float64)
    n = Y.shape[0]
    Zsum = 0.0
    rep = np.zeros((n, 2))
    want = np.zeros(n, bool)
    want[np.arange(n) if rows is None else rows] = True
    for s in range(0, n, 512):
        d = Y[s:s + 512, None, :] - Y[None, :, :]
        w = 1.0 / (1.0 + (d ** 2).sum(axis=2))
        w[np.arange(d.shape[0]), np.arange(s, s + d.shape[0])] = 0.0
        Zsum += w.sum()
        sel = want[s:s + 512]
        if sel.any():
            rep[s:s + 512][sel] = ((w[sel] ** 2)[:, :, None] * d[sel]).sum(axis=1)
    src = np.repeat(np.arange(n), np.diff(indptr))
    p = vals * exaggeration
    d = Y[src] - Y[cols]
    w = 1.0 / (1.0 + (d ** 2).sum(axis=1))
    att = np.zeros((n, 2))
    np.add.at(att, src, (p * w)[:, None] * d)
    kl = float(np.sum(p * np.log(np.maximum(p, MACHINE_EPSILON) / np.maximum(w / Zsum, MACHINE_EPSILON))))
    grad = 4.0 * (att - rep / Zsum)
    return kl, (grad if rows is None else grad[rows])


def gradient_descent(Y0, csr, it, max_iter, exaggeration, momentum, learning_rate, min_gain=0.01, n_iter_check=50,
                     n_iter_without_progress=300, min_grad_norm=1e-7):
    """sklearn/manifold/_t_sne.py _gradient_descent: (Y, error, last iteration)."""
    p = np.array(Y0, np.float64)
    update, gains = np.zeros_like(p), np.ones_like(p)
    error = best_error = np.finfo(float).max
    best_iter = i = it
    for i in range(it, max_iter):
        check = (i + 1) % n_iter_check == 0
        error_i, grad = kl_gradient(p, csr, exaggeration)
        if check or i == max_iter - 1:
            error = error_i
        inc = update * grad < 0.0
        gains[inc] += 0.2
        gains[~inc] *= 0.8
        np.clip(gains, min_gain, np.inf, out=gains)
        grad = grad * gains
        update = momentum * update - learning_rate * grad
        p = p + update
        if check:
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > n_iter_without_progress:
                break
            if np.linalg.norm(grad) <= min_grad_norm:
                break
    return p, error, i


def descend(Y0, csr, n_steps, exaggeration=1.0, momentum=0.8, learning_rate=200.0, min_gain=0.01):
    return gradient_descent(Y0, csr, 0, n_steps, exaggeration, momentum, learning_rate, min_gain, n_iter_check=1 << 62)[0]


def tsne(Y0, csr, early_exaggeration, learning_rate, max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7):
    """TSNE._tsne: (Y, KL, n_iter)."""
    Y, err, it = gradient_descent(Y0, csr, 0, 250, early_exaggeration, 0.5, learning_rate, n_iter_without_progress=250,
                                  min_grad_norm=min_grad_norm)
    if it < 250 or max_iter > 250:
        Y, err, it = gradient_descent(Y, csr, it + 1, max_iter, 1.0, 0.8, learning_rate,
                                      n_iter_without_progress=n_iter_without_progress, min_grad_norm=min_grad_norm)
    return Y, err, it


def trustworthiness(X, Y, n_neighbors=12):
    """sklearn.manifold.trustworthiness (euclidean), restated."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    n = X.shape[0]

    def dist(A):
        sq = (A ** 2).sum(axis=1)
        D = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * A @ A.T, 0.0))
        np.fill_diagonal(D, np.inf)
        return D
    ind_X = np.argsort(dist(X), axis=1, kind="stable")
    ind_Y = np.argsort(dist(Y), axis=1, kind="stable")[:, :n_neighbors]
    inv = np.zeros((n, n), dtype=np.int64)
    inv[np.arange(n)[:, None], ind_X] = np.arange(1, n + 1)
    ranks = inv[np.arange(n)[:, None], ind_Y] - n_neighbors
    t = float(np.sum(ranks[ranks > 0]))
    return 1.0 - t * (2.0 / (n * n_neighbors * (2.0 * n - 3.0 * n_neighbors - 1.0)))


# ---- inputs shared by the fixture generator and the tests ---------------------------------------------------------------
# (seed, n, d, perplexity): synthetic rows; k = min(n - 1, int(3 perplexity + 1)).  n = k + 2, tile edges 63 / 64 / 65 / 129,
# k = n - 1 (perplexity near n / 3), d in {2, 3, 50, 256}.  Every case carries 3 exact duplicate rows.
SHAPE_CASES = [(1, 18, 3, 5.0), (2, 63, 2, 10.0), (3, 64, 50, 21.0), (4, 65, 3, 21.5), (5, 129, 50, 30.0), (6, 257, 256, 30.0),
               (7, 40, 2, 13.0)]
LARGE_CASE = (8, 8448, 50, 30.0)   # three query batches of the neighbour search, 33 column ranges of the gradient


def synthetic(seed, n, d):
    """Three Gaussian blobs, seeded, the last 3 rows exact copies of rows 0, 1, 2."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)) + 4.0 * rng.standard_normal((3, d))[rng.integers(0, 3, n)]
    X[n - 3:] = X[:3]
    return X


def reference_rows(golden_dir, n_each):
    """n_each rows of each reference matrix of tests/golden/ref_features.npz, normalised (float64 counts / row sum); the
    positive rows start with the matrix's exact duplicate rows."""
    import os
    with np.load(os.path.join(golden_dir, "ref_features.npz")) as z:
        pos, neg = z["pos_counts"].astype(np.float64), z["neg_counts"].astype(np.float64)
    _, inv, cnt = np.unique(pos, axis=0, return_inverse=True, return_counts=True)
    dup = np.flatnonzero(cnt[inv.ravel()] > 1)
    rest = np.setdiff1d(np.arange(pos.shape[0]), dup)
    order = np.concatenate((dup, rest))[:n_each]
    X = np.vstack((pos[order], neg[:n_each]))
    return X / X.sum(axis=1, keepdims=True)
