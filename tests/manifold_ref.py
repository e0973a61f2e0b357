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
def binary_search_perplexity(d2, perplexity, margins=False):
    """sklearn/manifold/_utils.pyx _binary_search_perplexity on float64 squared distances: (P, beta).  The target is
    log(float32(perplexity)), scikit-learn's argument being a C float.  ``margins``: also, per row, the smallest
    | |diff| - 1e-5 | over the steps it took -- how far the row's stopping decisions are from flipping under another exp."""
    d2 = np.asarray(d2, np.float64)
    n, k = d2.shape
    target = np.log(float(np.float32(perplexity)))
    P = np.zeros((n, k))
    beta_out = np.empty(n)
    margin = np.full(n, np.inf)
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
            margin[i] = min(margin[i], abs(abs(diff) - 1e-5))
            if abs(diff) <= 1e-5:
                break
            if diff > 0.0:
                bmin = beta
                beta = beta * 2.0 if bmax == np.inf else (beta + bmax) / 2.0
            else:
                bmax = beta
                beta = beta / 2.0 if bmin == -np.inf else (beta + bmin) / 2.0
        P[i], beta_out[i] = p, beta
    return (P, beta_out, margin) if margins else (P, beta_out)


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
                     n_iter_without_progress=300, min_grad_norm=1e-7, log=None):
    """sklearn/manifold/_t_sne.py _gradient_descent: (Y, error, last iteration).  ``log``: a list that receives one
    (iteration, error, best error before the check, gradient norm, iterations since the best after the check, limit,
    min_grad_norm) per check."""
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
            if log is not None:
                log.append((i, error, best_error, float(np.linalg.norm(grad)), i - (i if error < best_error else best_iter),
                            n_iter_without_progress, min_grad_norm))
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > n_iter_without_progress:
                break
            if np.linalg.norm(grad) <= min_grad_norm:
                break
    return p, error, i


def descend(Y0, csr, n_steps, exaggeration=1.0, momentum=0.8, learning_rate=200.0, min_gain=0.01):
    return gradient_descent(Y0, csr, 0, n_steps, exaggeration, momentum, learning_rate, min_gain, n_iter_check=1 << 62)[0]


def tsne(Y0, csr, early_exaggeration, learning_rate, max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7, log=None):
    """TSNE._tsne: (Y, KL, n_iter).  ``log``: see gradient_descent; both phases append to it."""
    Y, err, it = gradient_descent(Y0, csr, 0, 250, early_exaggeration, 0.5, learning_rate, n_iter_without_progress=250,
                                  min_grad_norm=min_grad_norm, log=log)
    if it < 250 or max_iter > 250:
        Y, err, it = gradient_descent(Y, csr, it + 1, max_iter, 1.0, 0.8, learning_rate,
                                      n_iter_without_progress=n_iter_without_progress, min_grad_norm=min_grad_norm, log=log)
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


# ---- references and inputs of tests/test_gpu_manifold_shapes.py (conditions on them: tests/test_manifold_host.py) -------
LD = np.longdouble


def covariance(X):
    """Two-pass mean and covariance in np.longdouble: (mean, cov, |Xc|^T |Xc|) -- the last is what a rounding bound of
    any summation of the products scales with."""
    X = np.asarray(X, np.float64).astype(LD)
    mean = X.sum(axis=0) / X.shape[0]
    Xc = X - mean
    return mean, Xc.T @ Xc / (X.shape[0] - 1), np.abs(Xc).T @ np.abs(Xc)


def covariance_one_pass(X):
    """(sum x x^T - n mean mean^T) / (n - 1) in float64: the formula the device does NOT use."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    mean = X.sum(axis=0) / n
    return (X.T @ X - n * np.outer(mean, mean)) / (n - 1)


def pca_chunk_rows(n, D):
    """tsne.hip's pca_chunk_rows: rows per chunk of the PCA sums."""
    cap = min(65535, max(1, (256 << 20) // (D * D * 8)))
    R = max(1024, -(-n // cap))
    return (R + 3) & ~3


def covariance_bound(n, D, abs_gram):
    """Elementwise bound on the device covariance: every entry is a sum of n products of centred values, accumulated in
    chains of at most R rows (one chunk, on the matrix pipe) and then over the chunks in order.  With u = eps / 2 the unit
    roundoff: each centred factor carries <= u, each product <= u, every addition <= u, so the entry is off by at most
    (R + chunks + 3) u sum|xc_a xc_b| (Higham, Accuracy and Stability, (3.5)).  The bound used is twice that -- c = 1 with
    eps in place of u -- and the spare half covers the second-order term n delta_a delta_b of the device mean's own error
    delta <= (R + chunks) u mean|x|."""
    R = pca_chunk_rows(n, D)
    chain = R + -(-n // R) + 3
    return chain * MACHINE_EPSILON * np.asarray(abs_gram, np.float64) / (n - 1), chain


def spectrum_data(seed, n, D, offset=0.0):
    """Gaussian rows whose column scales fall geometrically (clear eigenvalue gaps at the top), plus a common offset."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, D)) * (0.8 ** np.minimum(np.arange(D), 40)) + offset


PCA_CASES = [(1023, 7, 0.0), (1024, 64, 0.0), (1025, 65, 0.0), (1027, 100, 0.0), (2049, 257, 0.0), (5000, 300, 0.0),
             (40, 100, 0.0), (3000, 16, 1e6)]
PCA_CAP_CASE = (2101, 4096)     # 256 MiB / (8 D^2) = 2 chunks at most: 1052 rows per chunk, above the floor of 1024


def lattice_rows(seed, n, side, d):
    """n rows drawn from the integer grid {0 .. side - 1}^d: every squared distance is a small integer, shared by many."""
    return np.random.default_rng(seed).integers(0, side, (n, d)).astype(np.float64)


# (seed, n, side, d, k): 64 cells x ~47 rows, 125 cells x ~24 rows, 16 cells x ~100 rows; k cuts a class of several hundred equal distances
LATTICE_CASES = [(21, 3001, 8, 2, 700), (22, 3001, 5, 3, 300), (23, 1601, 4, 2, 900)]


def tie_cut(Drow, k):
    """For one row of squared distances (self = inf): (members of the class of the k-th smallest value, how many of them
    the selection takes)."""
    T = np.partition(Drow, k - 1)[k - 1]
    members = np.flatnonzero(Drow == T)
    return members, k - int(np.sum(Drow < T))


def affinity_edge_cases():
    """(name, d2, perplexity) of the perplexity-search edge tests: sorted positive rows as a neighbour search gives them,
    scaled by 1e6 (every exp underflows at beta = 1: the sum_p == 0 branch, then halving) and 1e-6 (doubling), and k = 4096."""
    rng = np.random.default_rng(31)
    base = np.sort(rng.chisquare(3, (400, 91)) + 0.05, axis=1)
    wide = np.sort(rng.chisquare(3, (64, 4096)) + 0.05, axis=1)
    return [("x1e6", base * 1e6, 30.0), ("x1e-6", base * 1e-6, 30.0), ("plain", base, 30.0), ("k4096", wide, 1365.0),
            ("k4096_p30", wide, 30.0)]


def control_problem():
    """(X, Y0) of the control-loop cases: 90 rows in three blobs, perplexity CONTROL_PERPLEXITY, the first two coordinates as
    the initial embedding (a start in the basin the descent contracts in -- from scikit-learn's 1e-4 start the symmetry
    breaking amplifies rounding by many orders of magnitude)."""
    X = synthetic(11, 90, 5)
    return X, np.ascontiguousarray(X[:, :2])


CONTROL_PERPLEXITY = 8.0
# name -> TSNE arguments.  Learning rates are low on purpose: at scikit-learn's 'auto' rate the gains rule makes a 90-row
# descent chaotic within a hundred steps (a 1e-13 change of the start moves the result by tenths of the span), and no
# tolerance could then hold the device to the restatement.  'stall' has learning rate 0: the embedding does not move, every
# check after a phase's first compares an error with itself, so the progress rule alone decides, with j - best_iter equal to
# the limit exactly at iteration 349 ('>' goes on to 399, '>=' would stop at 349).
CONTROL_CASES = {
    "max_iter_250": dict(early_exaggeration=1.0, learning_rate=5.0, max_iter=250),
    "max_iter_251": dict(early_exaggeration=12.0, learning_rate=1.0, max_iter=251),
    "max_iter_333": dict(early_exaggeration=1.0, learning_rate=5.0, max_iter=333),
    "full_1000": dict(early_exaggeration=1.0, learning_rate=2.0, max_iter=1000),
    "grad_norm_phase_1": dict(early_exaggeration=12.0, learning_rate=1.0, max_iter=1000, min_grad_norm=1e3),
    "grad_norm_phase_2": dict(early_exaggeration=1.0, learning_rate=5.0, max_iter=1000, min_grad_norm=0.03),
    "stall": dict(early_exaggeration=1.0, learning_rate=0.0, max_iter=1000, n_iter_without_progress=50),
}
CONTROL_EXPECTED_N_ITER = {"max_iter_250": 250, "max_iter_251": 250, "max_iter_333": 332, "full_1000": 999,
                           "grad_norm_phase_1": 99, "grad_norm_phase_2": 299, "stall": 399}


def control_reference(name, log=None):
    """ref.tsne of a control case on the restatement's own affinities: (Y, KL, n_iter)."""
    X, Y0 = control_problem()
    k = min(X.shape[0] - 1, int(3 * CONTROL_PERPLEXITY + 1))
    idx, d2 = neighbors(X, k)
    csr = symmetrize(idx, binary_search_perplexity(d2, CONTROL_PERPLEXITY)[0])
    kw = dict(CONTROL_CASES[name])
    return tsne(Y0, csr, kw.pop("early_exaggeration"), kw.pop("learning_rate"), log=log, **kw)


def decision_margins(log, moved=True):
    """The smallest relative margin of the decisions of a check log: error < best and grad_norm <= min_grad_norm.  Where
    the embedding did not move (learning rate 0) an error equal to the best is the same number computed twice, not a close
    call, and is left out."""
    m = np.inf
    for (i, error, best, gnorm, since, limit, min_gn) in log:
        if moved or error != best:
            m = min(m, abs(error - best) / max(abs(error), abs(best)))
        if min_gn > 0:
            m = min(m, abs(gnorm - min_gn) / max(gnorm, min_gn))
    return m


def lattice_embedding(seed, n, side):
    """(Y (n, 2), cells (side^2, 2), counts): n points on the cells of a side x side integer grid, seeded multiplicities."""
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, side * side, n)
    cells = np.stack(np.divmod(np.arange(side * side), side), axis=1).astype(np.float64)
    return cells[cell], cells, np.bincount(cell, minlength=side * side)


def ring_csr(n, seed):
    """A sparse P for large n: up to three entries per row (i + 1, i + 7919 or i + n // 3, a seeded column; wrapped), values summing to 1."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    far = 7919 if n > 2 * 7919 else n // 3
    cols = np.sort(np.stack(((i + 1) % n, (i + far) % n, (i + rng.integers(2, n - 1, n)) % n), axis=1), axis=1)
    keep = np.concatenate((np.ones((n, 1), bool), cols[:, 1:] != cols[:, :-1]), axis=1) & (cols != i[:, None])
    indptr = np.concatenate(([0], np.cumsum(keep.sum(axis=1)))).astype(np.int64)
    vals = rng.random(int(indptr[-1])) + 0.5
    return indptr, cols[keep].astype(np.int32), vals / vals.sum()


def kl_gradient_lattice(Y, cells, counts, csr, rows, exaggeration=1.0):
    """(KL, grad of ``rows``, Z, sum |repulsive terms| of ``rows`` (len, 2), sum |attractive terms| (len, 2), sum |KL terms|)
    for an embedding whose points lie on ``cells`` with multiplicities ``counts``, in np.longdouble:
    Z = sum_ab c_a c_b w(a - b) - n (O(cells^2)), r_i = sum_b c_b w^2 (y_i - y_b) (O(cells) per row)."""
    indptr, cols, vals = csr
    Y = np.asarray(Y, np.float64)
    n = Y.shape[0]
    C, c = cells.astype(LD), counts.astype(LD)
    Z = LD(0)
    for s in range(0, len(C), 256):
        d = C[s:s + 256, None, :] - C[None, :, :]
        Z += ((1 / (1 + (d ** 2).sum(axis=2))) * c[None, :] * c[s:s + 256, None]).sum()
    Z -= n
    d = Y[rows].astype(LD)[:, None, :] - C[None, :, :]
    w2 = (1 / (1 + (d ** 2).sum(axis=2))) ** 2 * c[None, :]
    rep = (w2[:, :, None] * d).sum(axis=1)
    rep_abs = (w2[:, :, None] * np.abs(d)).sum(axis=1)
    src = np.repeat(np.arange(n), np.diff(indptr))
    p = vals.astype(LD) * exaggeration
    de = Y[src].astype(LD) - Y[cols].astype(LD)
    w = 1 / (1 + (de ** 2).sum(axis=1))
    terms = p * np.log(np.maximum(p, MACHINE_EPSILON) / np.maximum(w / Z, MACHINE_EPSILON))
    att, att_abs = np.zeros((len(rows), 2), LD), np.zeros((len(rows), 2), LD)
    for a, i in enumerate(rows):
        e = slice(indptr[i], indptr[i + 1])
        att[a] = ((p[e] * w[e])[:, None] * de[e]).sum(axis=0)
        att_abs[a] = ((p[e] * w[e])[:, None] * np.abs(de[e])).sum(axis=0)
    return terms.sum(), 4 * (att - rep / Z), Z, rep_abs, att_abs, np.abs(terms).sum()


def gradient_ranges(n):
    """tsne.hip's column ranges of the gradient: (tiles, G, [first row of range g for g in 0..G])."""
    tiles = -(-n // 256)
    G = min(max(1, -(-2048 // tiles)), tiles)
    return tiles, G, [min(n, 256 * (tiles * g // G)) for g in range(G + 1)]
