"""The statement of the mixture E-step in float64 and in ``longdouble``, the reduction rule of the
device written out, and the error bound.  Nothing here imports the library.

    S[i,k] = sum_j c_i[j] log theta_k[j] + log pi_k      l_i = logsumexp_k S[i,k]      r[i,k] = exp(S[i,k] - l_i)
    T[k,j] = sum_i r[i,k] c_i[j]      N_k = sum_i r[i,k]      L = sum_i l_i

Reduction rule of the device: rows in blocks of BLOCK_ROWS consecutive rows anchored at row 0; inside a block a column of
T meets its rows four at a time in row order (one matrix instruction per four rows); the blocks' results are folded by the
tree of tests/segment_fit_ref.py (256 consecutive entries, v[i] += v[i + s] for s = 128 .. 1, level after level).  The
longest path therefore holds t = BLOCK_ROWS + 8 * levels additions."""
import numpy as np

U = 2.0 ** -53
BLOCK_ROWS = 1024
TREE = 256
TINY = 2.0 ** -1000


def tree_levels(blocks):
    levels = 1
    while blocks > TREE:
        blocks = -(-blocks // TREE)
        levels += 1
    return levels


def path_additions(n_rows):
    """t of the bound: the additions on the longest path of the row reduction."""
    return BLOCK_ROWS + 8 * tree_levels(max(1, -(-n_rows // BLOCK_ROWS)))


def tree_sum(values):
    """The sums over axis 0 of ``values`` (R, ...) float64 by the fixed tree, written out."""
    v = np.array(values, dtype=np.float64)
    while True:
        blocks = max(1, -(-v.shape[0] // TREE))
        padded = np.zeros((blocks * TREE,) + v.shape[1:])
        padded[:v.shape[0]] = v
        w = padded.reshape((blocks, TREE) + v.shape[1:])
        s = TREE // 2
        while s:
            w[:, :s] += w[:, s:2 * s]
            s //= 2
        v = w[:, 0].copy()
        if blocks == 1:
            return v[0]


def block_sums(values):
    """One partial per block of BLOCK_ROWS rows of ``values`` (N, ...) float64, anchored at row 0, in the order of
    ``mix_expect_body``'s N_k and L: lane group kk = 0 .. 3 of the wave (row slot s) starts from +0.0 and adds rows
    b * BLOCK_ROWS + s, + 4, + 8, ... in row order, a row past N as +0.0; the two ``__shfl_xor`` steps (16, then 32) join the
    slots as (0 + 1) + (2 + 3).  ``tree_sum(block_sums(x))`` is the device's N_k for x = r (N, K) and its L for x = l (N,)."""
    v = np.asarray(values, dtype=np.float64)
    n = v.shape[0]
    blocks = max(1, -(-n // BLOCK_ROWS))
    padded = np.zeros((blocks * BLOCK_ROWS,) + v.shape[1:])
    padded[:n] = v
    steps = padded.reshape((blocks, BLOCK_ROWS // 4, 4) + v.shape[1:])
    slots = np.zeros((blocks, 4) + v.shape[1:])
    for i in range(BLOCK_ROWS // 4):
        slots += steps[:, i]
    return (slots[:, 0] + slots[:, 1]) + (slots[:, 2] + slots[:, 3])


def device_order(r, l):
    """(N_k, L) of the device from its own r (N, K) and l (N,): both are plain float64 adds, so this is exact."""
    return tree_sum(block_sums(r)), float(tree_sum(block_sums(l)))


def two_profile_case(n_rows, K, seed=4):
    """(counts (n_rows, 4) uint32, log_profiles (K, 4), log_w (K,)): the inputs of the two-level tests, shared by the GPU
    tests and the host's discrimination checks.  Rows of 30 k-mers from two planted profiles, each row's profile a fair coin;
    the table is the same profiles lightly perturbed (K = 1: the first alone), so that neither component starves.  Seed 4 is
    the first at which every order tests/test_mixture_host.py sets against the device's gives other bits on the float64
    statement's r and l (at seeds 1 to 3 one of the two plain sums of l happens to round to the device's L)."""
    rng = np.random.RandomState(seed)
    planted_profiles = np.array([[0.40, 0.30, 0.20, 0.10], [0.10, 0.20, 0.30, 0.40]])
    label = rng.randint(0, 2, n_rows).astype(bool)
    counts = np.where(label[:, None], rng.multinomial(30, planted_profiles[1], n_rows),
                      rng.multinomial(30, planted_profiles[0], n_rows)).astype(np.uint32)
    table = planted_profiles[:K] * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (K, 4)))
    table /= table.sum(axis=1, keepdims=True)
    weights = np.array([0.45, 0.55])[:K]
    return counts, np.log(table), np.log(weights / weights.sum())


def e_step(counts, log_profiles, log_w, dtype=np.longdouble):
    """dict(l, r, T, Nk, L, argmax, max_resp) of one E-step in ``dtype``; float64: T, N_k and L by blocks and tree."""
    c = np.asarray(counts).astype(dtype)
    lp = np.asarray(log_profiles, dtype=np.float64).astype(dtype)
    lw = np.asarray(log_w, dtype=np.float64).astype(dtype)
    S = c @ lp.T + lw[None, :]
    m = S.max(axis=1)
    with np.errstate(under='ignore'):
        l = m + np.log(np.exp(S - m[:, None]).sum(axis=1))
        r = np.exp(S - l[:, None])
    if dtype == np.float64:
        blocks = range(0, max(len(c), 1), BLOCK_ROWS)
        T = tree_sum([r[b:b + BLOCK_ROWS].T @ c[b:b + BLOCK_ROWS] for b in blocks])
        Nk = tree_sum([r[b:b + BLOCK_ROWS].sum(axis=0) for b in blocks])
        L = tree_sum([l[b:b + BLOCK_ROWS].sum() for b in blocks])
    else:
        T, Nk, L = r.T @ c, r.sum(axis=0), l.sum()
    return dict(l=l, r=r, T=T, Nk=Nk, L=L, argmax=np.argmax(r, axis=1), max_resp=r.max(axis=1))


def bounds(counts, log_profiles, exact):
    """dict(l (N,), T (K, D), Nk (K,), L) of the issue's bound around the extended statement ``exact``."""
    c = np.asarray(counts).astype(np.float64)
    lp = np.asarray(log_profiles, dtype=np.float64)
    N, D = c.shape
    K = lp.shape[0]
    e = (D + 2) * U * (c @ np.abs(lp).T).max(axis=1)
    rho = np.expm1(2 * e) + (K + 64) * U
    t = path_additions(N)
    l = exact["l"].astype(np.float64)
    r = exact["r"].astype(np.float64)
    b_l = e + (K + 64) * U * (1 + np.abs(l))
    f = rho + (t + 2) * U
    return dict(l=b_l, T=(r * f[:, None]).T @ c + TINY, Nk=(r * f[:, None]).sum(axis=0) + TINY,
                L=b_l.sum() + (t + 2) * U * np.abs(l).sum(), e=e, rho=rho)


def within(got, exact, bound):
    """The largest |got - exact| / bound (<= 1: inside)."""
    d = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(exact, dtype=np.longdouble))
    return float(np.max(d / np.asarray(bound, dtype=np.longdouble))) if np.size(d) else 0.0


def check_e_step(got, counts, log_profiles, log_w):
    """Asserts a dict(T, Nk, L, l) (any subset) within the bound of the extended statement; returns the largest ratio."""
    exact = e_step(counts, log_profiles, log_w)
    b = bounds(counts, log_profiles, exact)
    worst = 0.0
    for name in ("l", "T", "Nk", "L"):
        if name in got:
            assert np.all(np.isfinite(got[name])), name
            ratio = within(got[name], exact[name], b[name])
            assert ratio <= 1.0, (name, ratio)
            worst = max(worst, ratio)
    return worst


class StatementEStep(object):
    """The float64 statement in the place of phamers_amd.mixture's device E-step (same calls)."""

    def __init__(self, counts, batch_rows=0):
        from phamers_amd.likelihood import _count_rows
        self.host = _count_rows(counts, "counts")
        self.n, self.D = self.host.shape
        self.calls = 0

    def rows(self, index):
        return self.host[index]

    def __call__(self, log_profiles, log_w, rows=False):
        self.calls += 1
        g = e_step(self.host, log_profiles, log_w, np.float64)
        out = (g["T"], g["Nk"], float(g["L"]))
        return out + ((g["l"], g["argmax"].astype(np.int32), g["max_resp"]) if rows else ())

    def responsibilities(self, log_profiles, log_w):
        g = e_step(self.host, log_profiles, log_w, np.float64)
        return g["r"], g["l"]

    def close(self):
        pass


def planted(seed, n_components, rows_each, kmers, concentration, D=256):
    """(counts (K * rows_each, D) uint32, labels): rows drawn from K Dirichlet(concentration * 1) profiles."""
    rng = np.random.RandomState(seed)
    profiles = rng.dirichlet(np.full(D, float(concentration)), n_components)
    counts = np.vstack([rng.multinomial(kmers, p, rows_each) for p in profiles]).astype(np.uint32)
    return counts, np.repeat(np.arange(n_components), rows_each)
