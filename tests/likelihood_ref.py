"""The multinomial likelihood score (phamers_amd/likelihood.py) restated twice -- NumPy float64 and
NumPy longdouble (64-bit mantissa on x86) -- and the tolerance the device and the float64 statement are held to.

    p_r[j]   = (x_r[j] + a) / (sum_j x_r[j] + D a)
    S[q, r]  = sum_j c_q[j] log p_r[j]
    l_C(q)   = logsumexp_{r in C, group(r) != group(q) or a group < 0} S[q, r] - log n_eff(q, C)
    score(q) = l_+(q) - l_-(q)

The scorer is a function of (count rows, float64 log table): ``statement`` therefore takes the float64 table as its input
(exact in either precision) and restates everything after it; ``log_table`` restates the table, and its own test compares
it with the logarithm taken in longdouble.

Tolerance (derived, not measured; u = 2^-53).  A float64 dot product of D terms, in any order and with or without fused
multiply-adds, errs by at most (D + 2) u sum_j |c_j| |log p_j| (the bound DESIGN.md section 4.5 uses), so
    e_C(q) = (D + 2) u max_{r in C} sum_j c_q[j] |log p_r[j]|
bounds the error of every S of class C.  A log-sum-exp moves by at most the largest change of its arguments; the sum of
at most M terms in (0, 1], the exp, the two logarithms and the final additions add a relative error of a few u to values
of magnitude 1 + |l|.  Hence
    |score - exact| <= 2 (e_+ + e_-) + 64 u (1 + |l_+| + |l_-|),
two e per class because both the value under test and a float64 reference may err, and the same bound serves l_+ and l_-.
The longdouble statement's own error is 2^-11 of this.
"""
import numpy as np

U = 2.0 ** -53
assert np.finfo(np.longdouble).nmant >= 63, "the extended statement needs a longdouble wider than float64"


def log_table(counts, pseudocount=0.5, dtype=np.float64):
    x = np.asarray(counts).astype(dtype)
    a = dtype(pseudocount)
    return np.log((x + a) / (x.sum(axis=1, keepdims=True) + dtype(x.shape[1]) * a))


def random_groups(seed, n):
    """n group ids drawn from -1 .. 5 (-1: no group), not periodic in the index: what one device batch sees is not what
    the next one sees, so a batch that read another batch's ids gives other results."""
    return np.random.default_rng(seed).integers(-1, 6, n)


def groups_of_the_first_batch(groups, batch_rows=128):
    """The ids a call split into batches of ``batch_rows`` would use if every batch read the first batch's: the mistake the
    tests of groups across batches are there to catch."""
    g = np.asarray(groups)
    return g[np.arange(len(g)) % batch_rows]


def _class_term(c, table, qg, g, dtype):
    """l_C of the count rows c (N, D) under the float64 log table (M, D), in ``dtype``."""
    S = c.astype(dtype) @ table.astype(dtype).T
    keep = np.ones(S.shape, dtype=bool)
    if qg is not None and g is not None:
        qg, g = np.asarray(qg), np.asarray(g)
        keep = ~((qg[:, None] >= 0) & (qg[:, None] == g[None, :]))
    n_eff = keep.sum(axis=1)
    if (n_eff == 0).any():
        raise ValueError("a query's group leaves a class without rows")
    S = np.where(keep, S, dtype(-np.inf))
    m = S.max(axis=1)
    return m + np.log(np.exp(S - m[:, None]).sum(axis=1)) - np.log(n_eff.astype(dtype))


def statement(query_counts, log_pos, log_neg=None, query_groups=None, groups_pos=None, groups_neg=None, dtype=np.float64):
    """(l_pos, l_neg, score) in ``dtype`` (np.float64 or np.longdouble); log_neg None: one class, l_neg = 0."""
    c = np.atleast_2d(np.asarray(query_counts))
    lp = _class_term(c, np.asarray(log_pos), query_groups, groups_pos, dtype)
    ln = np.zeros(len(c), dtype=dtype) if log_neg is None else _class_term(c, np.asarray(log_neg), query_groups, groups_neg, dtype)
    return lp, ln, lp - ln


def tolerance(query_counts, log_pos, log_neg, l_pos, l_neg):
    """The bound of the module docstring, (N,) float64, for results near (l_pos, l_neg)."""
    c = np.atleast_2d(np.asarray(query_counts)).astype(np.float64)
    D = c.shape[1]
    e = (D + 2) * U * (c @ np.abs(np.asarray(log_pos)).T).max(axis=1)
    if log_neg is not None:
        e = e + (D + 2) * U * (c @ np.abs(np.asarray(log_neg)).T).max(axis=1)
    return 2.0 * e + 64.0 * U * (1.0 + np.abs(np.asarray(l_pos, dtype=np.float64)) + np.abs(np.asarray(l_neg, dtype=np.float64)))


def check(got, query_counts, log_pos, log_neg=None, query_groups=None, groups_pos=None, groups_neg=None, what=""):
    """Asserts that ``got`` -- (l_pos, l_neg, score), or the scores alone -- lies within the bound of the extended statement;
    returns (extended statement, bound)."""
    want = statement(query_counts, log_pos, log_neg, query_groups, groups_pos, groups_neg, dtype=np.longdouble)
    tol = tolerance(query_counts, log_pos, log_neg, want[0], want[1])
    pairs = zip(("l_pos", "l_neg", "score"), got, want) if isinstance(got, tuple) else [("score", got, want[2])]
    for name, g, w in pairs:
        err = np.abs(np.asarray(g).astype(np.longdouble) - w).astype(np.float64)
        worst = int(np.argmax(err / tol))
        assert (err <= tol).all(), "%s %s: row %d off by %.3e, bound %.3e" % (what, name, worst, err[worst], tol[worst])
    return want, tol
