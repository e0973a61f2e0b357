"""The likelihood-ranked reference lookup (phamers_amd/hosts.py) restated in NumPy float64 and NumPy
longdouble (64-bit mantissa on x86), and the tolerances the device is held to.

    multinomial  L[r, j]      = log((x_r[j] + a) / (sum_j x_r[j] + D a))
    markov       L[r, 4p + b] = log((x_r[4p + b] + a) / (sum_b' x_r[4p + b'] + 4a))
    S[q, r]      = sum_j c_q[j] L[r, j]
    ranking(q)   = the first `top` rows r that q's group does not exclude, in order of (S descending, r ascending)
    l[p, r]      = S[p, r] / n_p,  mu[r] = mean_p l[p, r],  sigma[r] = sqrt(sum_p (l[p, r] - mu[r])^2 / (P - 1))

The device is a function of (count rows, float64 log table); the statements below therefore take the float64 table as
their input (exact in either precision) and restate what comes after it.

Tolerances (derived, not measured; u = 2^-53).

S.  A float64 dot product of D terms, in any order and with or without fused multiply-adds, errs by at most
(D + 2) u sum_j |c_j| |L_j| (the bound DESIGN.md section 4.5 uses; tests/likelihood_ref.py), so
    e(q) = (D + 2) u max_r sum_j c_q[j] |L[r, j]|
bounds the error of every S of query q.  The longdouble statement's own error is 2^-11 of this.

Ranking.  The device orders its own S values.  With |S_dev - S| <= e(q): a row that was not returned has
S_dev <= S_dev(last returned), hence S <= S(last returned) + 2 e(q); and where the exact gaps among the true first
top + 1 rows all exceed 2 e(q), no error within e(q) can change the order or the membership of the first top: the indices
are then the true ones exactly.

mu.  l[p, r] carries e(p) / n_p from S plus one rounding of the division, u |l|.  The sum of P terms in row order adds at
most (P - 1) u sum_p |l| (every partial sum is bounded by sum |l|), the division by P one more rounding:
    t_mu[r] = mean_p e(p) / n_p + (P + 1) u mean_p |l[p, r]| + u |mu[r]|.

sigma.  sigma = |d|_2 / sqrt(P - 1) with d_p = l[p, r] - mu[r].  The computed d_p errs by at most
    delta_p = e(p) / n_p + u |l[p, r]| + t_mu[r] + u |d_p|
(the term, the mean the device centres on, the subtraction), and | |d^|_2 - |d|_2 | <= |d^ - d|_2 <= sqrt(P) max_p delta_p.
The sum of P non-negative squares by fused multiply-adds has a relative error of at most P u, the division and the square
root add 2 u; the root halves a relative error:
    t_sigma[r] = sqrt(P / (P - 1)) max_p delta_p + (P / 2 + 2) u sigma[r].
"""
import numpy as np

U = 2.0 ** -53
assert np.finfo(np.longdouble).nmant >= 63, "the extended statement needs a longdouble wider than float64"


def log_table(counts, pseudocount=0.5, dtype=np.float64):
    x = np.asarray(counts).astype(dtype)
    a = dtype(pseudocount)
    return np.log((x + a) / (x.sum(axis=1, keepdims=True) + dtype(x.shape[1]) * a))


def markov_log_table(counts, pseudocount=0.5, dtype=np.float64):
    x = np.asarray(counts).astype(dtype)
    M, D = x.shape
    a = dtype(pseudocount)
    g = x.reshape(M, D // 4, 4)
    return np.log((g + a) / (g.sum(axis=2, keepdims=True) + dtype(4) * a)).reshape(M, D)


def table(counts, model, pseudocount=0.5, dtype=np.float64):
    return (markov_log_table if model == 'markov' else log_table)(counts, pseudocount, dtype)


def products(query_counts, L, dtype=np.longdouble):
    """S (N, M) in ``dtype``."""
    return np.atleast_2d(np.asarray(query_counts)).astype(dtype) @ np.asarray(L).astype(dtype).T


def bound(query_counts, L):
    """e(q) of the module docstring, (N,) float64."""
    c = np.atleast_2d(np.asarray(query_counts)).astype(np.float64)
    return (c.shape[1] + 2) * U * (c @ np.abs(np.asarray(L, dtype=np.float64)).T).max(axis=1)


def excluded(query_groups, reference_groups, N, M):
    """(N, M) bool: the pairs a ranking leaves out."""
    if query_groups is None or reference_groups is None:
        return np.zeros((N, M), dtype=bool)
    qg, rg = np.asarray(query_groups), np.asarray(reference_groups)
    return (qg[:, None] >= 0) & (qg[:, None] == rg[None, :])


def random_groups(seed, n):
    """n group ids drawn from -1 .. 5 (-1: no group), not periodic in the index: what one device batch sees is not what
    the next one sees, so a batch that read another batch's ids gives other results."""
    return np.random.default_rng(seed).integers(-1, 6, n)


def groups_of_the_first_batch(groups, batch_rows=128):
    """The ids a call split into batches of ``batch_rows`` would use if every batch read the first batch's: the mistake the
    tests of groups across batches are there to catch."""
    g = np.asarray(groups)
    return g[np.arange(len(g)) % batch_rows]


def ranking(S, top, out=None):
    """(indices (N, top), values (N, top)) of the statement: rows by (S descending, index ascending), ``out`` (N, M) bool
    left out."""
    S = np.asarray(S)
    idx = np.empty((S.shape[0], top), dtype=np.int64)
    for q in range(S.shape[0]):
        rows = np.arange(S.shape[1]) if out is None else np.flatnonzero(~out[q])
        order = rows[np.lexsort((rows, -S[q, rows]))]
        idx[q] = order[:top]
    return idx, np.take_along_axis(S, idx, axis=1)


def check_ranking(indices, values, S, e, top, out=None, what=""):
    """The four statements of a ranking against the longdouble products S (N, M) and the bound e (N,): every returned S
    within e of S at the returned index; the list sorted by (-S, index); every row not returned at most 2 e above the last
    returned; and, where the gaps among the true first top + 1 all exceed 2 e, the true indices exactly.  Returns the
    share of queries the last, exact check covered."""
    N, M = S.shape
    assert indices.shape == (N, top) and values.shape == (N, top) and indices.dtype == np.int64 and values.dtype == np.float64
    out = np.zeros((N, M), dtype=bool) if out is None else out
    want_idx, _ = ranking(S, min(top + 1, int((~out).sum(axis=1).min())), out)
    exact = 0
    for q in range(N):
        i, v = indices[q], values[q]
        assert ((i >= 0) & (i < M)).all() and len(set(i.tolist())) == top and not out[q, i].any(), (what, q, i)
        err = np.abs(v.astype(np.longdouble) - S[q, i]).astype(np.float64)
        assert (err <= e[q]).all(), "%s query %d: S off by %.3e, bound %.3e" % (what, q, err.max(), e[q])
        assert all(v[a] > v[a + 1] or (v[a] == v[a + 1] and i[a] < i[a + 1]) for a in range(top - 1)), (what, q, i, v)
        rest = ~out[q]
        rest[i] = False
        if rest.any():
            assert float(S[q, rest].max() - S[q, i[-1]]) <= 2.0 * e[q], (what, q)
        first = S[q, want_idx[q]]
        if len(first) < 2 or float((first[:-1] - first[1:]).min()) > 2.0 * e[q]:
            exact += 1
            assert np.array_equal(i, want_idx[q, :top]), (what, q, i, want_idx[q])
    return exact / float(N)


def null_statement(null_counts, L, dtype=np.longdouble):
    """(mu (M,), sigma (M,), l (P, M)) in ``dtype``; float64: every column summed in row order, as the device sums it."""
    c = np.asarray(null_counts)
    n = c.sum(axis=1).astype(dtype)
    ell = products(c, L, dtype) / n[:, None]
    P = dtype(len(c))
    mu = np.add.accumulate(ell, axis=0)[-1] / P
    d = ell - mu[None, :]
    sigma = np.sqrt(np.add.accumulate(d * d, axis=0)[-1] / (P - dtype(1)))
    return mu, sigma, ell


def null_tolerance(null_counts, L, mu, sigma, ell):
    """(t_mu (M,), t_sigma (M,)) of the module docstring, float64, around the extended statement (mu, sigma, ell)."""
    c = np.asarray(null_counts)
    P = len(c)
    per_row = bound(c, L) / c.sum(axis=1).astype(np.float64)            # e(p) / n_p
    ell, mu, sigma = (np.asarray(v, dtype=np.float64) for v in (ell, mu, sigma))
    a = np.abs(ell)
    t_mu = per_row.mean() + (P + 1) * U * a.mean(axis=0) + U * np.abs(mu)
    delta = (per_row[:, None] + U * a + t_mu[None, :] + U * np.abs(ell - mu[None, :])).max(axis=0)
    t_sigma = np.sqrt(P / (P - 1.0)) * delta + (P / 2.0 + 2.0) * U * sigma
    return t_mu, t_sigma


def check_null(mu, sigma, null_counts, L, what=""):
    want_mu, want_sigma, ell = null_statement(null_counts, L, np.longdouble)
    t_mu, t_sigma = null_tolerance(null_counts, L, want_mu, want_sigma, ell)
    for name, got, want, tol in (("mu", mu, want_mu, t_mu), ("sigma", sigma, want_sigma, t_sigma)):
        assert got.shape == want.shape and got.dtype == np.float64
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        worst = int(np.argmax(err / tol))
        assert (err <= tol).all(), "%s %s: row %d off by %.3e, bound %.3e" % (what, name, worst, err[worst], tol[worst])
    return t_mu, t_sigma


def z_and_p(per_kmer, indices, mu, sigma):
    """The host formula of hosts.py on returned pairs."""
    import math
    with np.errstate(invalid='ignore', divide='ignore'):
        z = (per_kmer - mu[indices]) / sigma[indices]
    p = np.array([0.5 * math.erfc(v / math.sqrt(2.0)) for v in z.ravel()]).reshape(z.shape)
    return z, p
